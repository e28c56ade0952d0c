// cam_kernels.h — the class-activation-map family as word saliencies.  Gradient forms (one launch per chunk of units, the
// gradient of lrp_decoder_gradient): Grad-CAM (Selvaraju et al., ICCV 2017), Grad-CAM++ (Chattopadhay et al., WACV 2018),
// XGrad-CAM (Fu et al., BMVC 2020), LayerCAM (Jiang et al., TIP 2021), HiResCAM (Draelos & Carin, 2020).  Gradient-free forms,
// whose channel weights come from forwards only: Score-CAM (Wang et al., CVPR-W 2020) and Ablation-CAM (Desai & Ramaswamy, WACV
// 2020).  In the style of gradcam_kernels.h / saliency_kernels.h: device pointers, one workgroup per unit (or per slice of a
// row), fixed-order wave + LDS reductions, fp64 accumulation, no float atomics: an output never depends on what else shares the
// launch.
//
//  cam_kernel           per unit u (image b = img_idx[u]), F = feat[b] (L, D), G = grads[u] (L, D), all in fp64:
//      mode 0 gradcam    w_c = (1/L) sum_l G[l][c];                                             A[l] = sum_c F[l][c] w_c
//      mode 1 gradcam++  S_c = sum_l F[l][c]; den = 2 G^2 + S_c G^3; alpha = den != 0 ? G^2 / den : 0;
//                        w_c = sum_l alpha[l][c] max(G[l][c], 0);                               A[l] = sum_c F[l][c] w_c
//      mode 2 xgradcam   w_c = sum_l F[l][c] G[l][c] / (sum_l F[l][c] + 1e-7);                  A[l] = sum_c F[l][c] w_c
//      mode 3 layercam   A[l] = sum_c max(G[l][c], 0) F[l][c]
//      mode 4 hirescam   A[l] = sum_c G[l][c] F[l][c]
//      then the finish of gradcam_kernel, statement for statement (cam_finish): cam = max(M A M^T, 0), cam /= max(cam) + 1e-6,
//      optional gate (double)gb * cam.  Mode 0 repeats gradcam_kernel's weight and A loops as well: the same bits.
//  cam_weighted_kernel  per (image i, word t): scores (n_img, R, T) fp64, row 0 the unmasked image, row 1 + k channel k,
//      row 1 + D the fill image (linear weights).  mode 0 softmax: w_k = exp(s_k - max) / sum exp(s - max), the sum taken by one
//      thread in ascending k; 1 linear: w_k = s_k - s_fill; 2 ablation: w_k = (s_0 - s_k) / |s_0|, all 0 where s_0 == 0.
//      A[l] = sum_c F[l][c] w_c, then cam_finish; the cam in fp64 and / or rounded once to float32.  A NaN score reaches every
//      A[l] of its own word (NaN * 0 is NaN) and nothing else.
//  scorecam_apply_kernel  row r = image img_idx[r] under the mask of channel k[r]: v[l] = feat[img][l][k] staged in LDS, min-max
//      normalised on the g x g grid in float32 ((v - min) / (max - min), each operation rounded on its own; zeros where max == min),
//      upsampled by exactly `up` pixels per cell with the half-pixel-centre bilinear rule of rise_mask (shift 0, rows and columns
//      clamped into [0, g - 1]), out = fill + m (x - fill) in the float32 rounding order of rise_apply_kernel.  k = -1 copies
//      the image, k = D gives the fill image; an image index outside [0, B) or a k outside [-1, D] gives a NaN row.
//      A workgroup takes one slice of CAM_SLICE groups of four values of one row and stages the channel itself: the slices of a
//      row share nothing.
//  feature_ablate_kernel  row r = feat[img_idx[r]] with channel k[r] set to 0, k = -1 a copy; an image index outside [0, B) or a
//      k outside [-1, D) gives a NaN row.
#pragma once
#include <hip/hip_runtime.h>
#include "gradcam_kernels.h"
#include "saliency_kernels.h"

namespace lrp {

enum { CAM_GRADCAM = 0, CAM_GRADCAMPP = 1, CAM_XGRADCAM = 2, CAM_LAYERCAM = 3, CAM_HIRESCAM = 4, CAM_MODES = 5 };
enum { CAMW_SOFTMAX = 0, CAMW_LINEAR = 1, CAMW_ABLATION = 2, CAMW_MODES = 3 };
constexpr int CAM_SLICE = 2048;           // groups of four values per workgroup of scorecam_apply_kernel

// A[l] = sum_c F[l][c] U[c]: one wave per position, lanes stride the channels (the loop of gradcam_kernel)
__device__ __forceinline__ void cam_fold_weights(const float* __restrict__ F, const double* U, double* A, int L, int D, int lane,
                                                 int wave) {
  for (int l = wave; l < L; l += 4) {
    double s = 0.0;
    for (int c = lane; c < D; c += 64) s += (double)F[(size_t)l * D + c] * U[c];
    s = wave_sum_d(s);
    if (lane == 0) A[l] = s;
  }
}

// one pixel of max(M U, 0), U = A M^T: the expression of gradcam_kernel's first pixel pass
__device__ __forceinline__ double cam_pixel(const double* U, const double* __restrict__ M, int g, int S, int p) {
  const int y = p / S, x = p - y * S;
  double s = 0.0;
  for (int i = 0; i < g; ++i) s += M[y * g + i] * U[i * S + x];
  return (s > 0.0 || s != s) ? s : 0.0;                     // np.maximum(cam, 0)
}

// The finish of gradcam_kernel from its second barrier on, in its order.  A (L) is complete and visible; U (>= g * S) is free.
// o: the unit's (S, S) fp64 cam, or null (the second pass then recomputes the pixel: the same expression, the same bits);
// gp / op: the unit's gate input and output (both or neither); o32: the cam rounded once, or null.
__device__ __forceinline__ void cam_finish(const double* A, double* U, const double* __restrict__ M, double* __restrict__ o,
                                           const float* __restrict__ gp, double* __restrict__ op, float* __restrict__ o32,
                                           double* red, int g, int S, int C, int tid, int lane, int wave) {
  const int npix = S * S;
  for (int q = tid; q < g * S; q += 256) {
    const int i = q / S, x = q - i * S;
    double s = 0.0;
    for (int j = 0; j < g; ++j) s += A[i * g + j] * M[x * g + j];
    U[q] = s;
  }
  __syncthreads();
  double mx = 0.0;
  for (int p = tid; p < npix; p += 256) {
    const double s = cam_pixel(U, M, g, S, p);
    if (o) o[p] = s;
    mx = s > mx ? s : mx;
  }
  mx = eval_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  const double den = fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) + 1e-6;
  for (int p = tid; p < npix; p += 256) {                   // same pixels per thread as the pass above
    const double v = (o ? o[p] : cam_pixel(U, M, g, S, p)) / den;
    if (o) o[p] = v;
    if (o32) o32[p] = (float)v;
    if (op) {
      const float* gq = gp + (size_t)p * C;
      double* oq = op + (size_t)p * C;
      for (int c = 0; c < C; ++c) oq[c] = (double)gq[c] * v;
    }
  }
}

// LDS: A (L) | U (max(D, g * S)), as gradcam_kernel
__global__ __launch_bounds__(256) void cam_kernel(const float* __restrict__ feat, const int* __restrict__ img_idx,
                                                  const float* __restrict__ grads, const double* __restrict__ M,
                                                  const float* __restrict__ gb, double* __restrict__ cams, double* __restrict__ outs,
                                                  int B, int g, int S, int D, int C, int mode) {
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
  if (mode <= CAM_XGRADCAM) {
    for (int c = tid; c < D; c += 256) {                    // channel weights: sequential over l, coalesced over c
      if (mode == CAM_GRADCAM) {
        double s = 0.0;
        for (int l = 0; l < L; ++l) s += (double)G[(size_t)l * D + c];
        U[c] = s / (double)L;
      } else {
        double sf = 0.0;
        for (int l = 0; l < L; ++l) sf += (double)F[(size_t)l * D + c];
        double w = 0.0;
        if (mode == CAM_GRADCAMPP) {
          for (int l = 0; l < L; ++l) {
            const double gv = (double)G[(size_t)l * D + c], g2 = gv * gv, g3 = g2 * gv;
            const double den = 2.0 * g2 + sf * g3;
            const double alpha = den != 0.0 ? g2 / den : 0.0;
            w += alpha * ((gv > 0.0 || gv != gv) ? gv : 0.0);
          }
          U[c] = w;
        } else {
          for (int l = 0; l < L; ++l) w += (double)F[(size_t)l * D + c] * (double)G[(size_t)l * D + c];
          U[c] = w / (sf + 1e-7);
        }
      }
    }
    __syncthreads();
    cam_fold_weights(F, U, A, L, D, lane, wave);
  } else {
    for (int l = wave; l < L; l += 4) {                     // no channel weights: the product is per position
      double s = 0.0;
      for (int c = lane; c < D; c += 64) {
        double gv = (double)G[(size_t)l * D + c];
        if (mode == CAM_LAYERCAM) gv = (gv > 0.0 || gv != gv) ? gv : 0.0;
        s += gv * (double)F[(size_t)l * D + c];
      }
      s = wave_sum_d(s);
      if (lane == 0) A[l] = s;
    }
  }
  __syncthreads();                                          // U changes its meaning here
  cam_finish(A, U, M, o, gb ? gb + u * npix * C : nullptr, outs ? outs + u * npix * C : nullptr, nullptr, red, g, S, C, tid,
             lane, wave);
}

// block = (image i, word t); LDS as cam_kernel
__global__ __launch_bounds__(256) void cam_weighted_kernel(const double* __restrict__ scores, const float* __restrict__ feat,
                                                           const int* __restrict__ img_idx, const double* __restrict__ M,
                                                           double* __restrict__ cams, float* __restrict__ maps,
                                                           int B, int R, int T, int g, int S, int D, int mode) {
  extern __shared__ double lds[];
  const int L = g * g;
  double* A = lds;
  double* U = lds + L;
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x, i = u / T;
  const int t = (int)(u - i * T);
  const int npix = S * S;
  double* o = cams ? cams + u * npix : nullptr;
  float* o32 = maps ? maps + u * npix : nullptr;
  const int b = img_idx[i];
  if (b < 0 || b >= B) {
    for (int p = tid; p < npix; p += 256) {
      if (o) o[p] = 0.0 / 0.0;
      if (o32) o32[p] = sal_nan();
    }
    return;
  }
  const float* F = feat + (size_t)b * L * D;
  const double* sc = scores + (i * R) * (size_t)T + t;      // row r of this word: sc[r * T]
  const double s0 = sc[0];
  if (mode == CAMW_SOFTMAX) {
    double mx = sc[(size_t)T];
    for (int c = tid; c < D; c += 256) {
      const double s = sc[(size_t)(1 + c) * T];
      mx = s > mx ? s : mx;
    }
    mx = eval_wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    for (int c = tid; c < D; c += 256) U[c] = exp(sc[(size_t)(1 + c) * T] - mx);
    __syncthreads();                                        // red[] was read above, U is complete
    if (tid == 0) {
      double s = 0.0;
      for (int c = 0; c < D; ++c) s += U[c];                // ascending k, one thread: the order depends on D alone
      red[0] = s;
    }
    __syncthreads();
    const double sum = red[0];
    for (int c = tid; c < D; c += 256) U[c] = U[c] / sum;
  } else if (mode == CAMW_LINEAR) {
    const double sf = sc[(size_t)(1 + D) * T];
    for (int c = tid; c < D; c += 256) U[c] = sc[(size_t)(1 + c) * T] - sf;
  } else {
    const double a0 = fabs(s0);
    for (int c = tid; c < D; c += 256) U[c] = s0 == 0.0 ? 0.0 : (s0 - sc[(size_t)(1 + c) * T]) / a0;
  }
  __syncthreads();                                          // (red[0] is read by every thread before cam_finish writes it)
  cam_fold_weights(F, U, A, L, D, lane, wave);
  __syncthreads();
  cam_finish(A, U, M, o, nullptr, nullptr, o32, red, g, S, 0, tid, lane, wave);
}

// a + f (b - a) with every operation rounded to float32 on its own.  The pragma keeps the compiler from fusing the product into
// the sum (the __f*_rn intrinsics are plain operators here and do not): tests/cam_ref.py restates this order bit for bit.
__device__ __forceinline__ float cam_lerp32(float a, float b, float f) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float p = f * d;
  return a + p;
}

struct ScoreCamGeom {
  int g, up, C, D;          // H = W = g * up
};

// grid (slices of a row, n rows); LDS: the channel's L = g * g normalised values
template <bool VEC>
__global__ __launch_bounds__(256) void scorecam_apply_kernel(const float* __restrict__ x, const float* __restrict__ feat,
                                                             const int* __restrict__ img_idx, const int* __restrict__ kk,
                                                             const float* __restrict__ fill, float* __restrict__ out, int B,
                                                             ScoreCamGeom q) {
  __shared__ float nv[EVAL_MAX_G * EVAL_MAX_G];
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = q.g * q.g, W = q.g * q.up;
  const size_t per = (size_t)W * W * q.C, groups = (per + 3) / 4;
  const size_t rr = blockIdx.y;
  const size_t g0 = (size_t)blockIdx.x * CAM_SLICE, g1 = g0 + CAM_SLICE < groups ? g0 + CAM_SLICE : groups;
  const int img = img_idx[rr], k = kk[rr];
  const bool bad = img < 0 || img >= B || k < -1 || k > q.D;
  const bool masked = !bad && k >= 0 && k < q.D;            // (wave- and block-uniform)
  if (masked) {
    const float* fp = feat + (size_t)img * L * q.D + k;
    float v = 0.f, lo = 0.f, hi = 0.f;
    if (tid < L) lo = hi = v = fp[(size_t)tid * q.D];       // L <= 256: one value per thread
    else lo = hi = fp[0];
    float a = lo, b = hi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ua = __shfl_xor(a, o, 64), ub = __shfl_xor(b, o, 64);
      a = ua < a ? ua : a;
      b = ub > b ? ub : b;
    }
    if (lane == 0) { red[wave] = a; red[4 + wave] = b; }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    if (tid < L) nv[tid] = hi == lo ? 0.f : (v - lo) / (hi - lo);     // (two differences and a division: nothing to fuse)
    __syncthreads();
  }
  for (size_t gi = g0 + tid; gi < g1; gi += 256) {
    const int e0 = (int)(4 * gi);
    const int lim = per - e0 < 4 ? (int)(per - e0) : 4;
    float* dst = out + rr * per + e0;
    float v[4];
    if (bad) {
      v[0] = v[1] = v[2] = v[3] = sal_nan();
    } else {
      int p = e0 / q.C, c = e0 - p * q.C, y = p / W, xx = p - y * W;
      if (k == q.D) {
        for (int e = 0; e < lim; ++e) { v[e] = fill[c]; if (++c == q.C) c = 0; }
      } else {
        const float* src = x + (size_t)img * per + e0;
        if (VEC) {
          const float4 t4 = *reinterpret_cast<const float4*>(src);
          v[0] = t4.x; v[1] = t4.y; v[2] = t4.z; v[3] = t4.w;
        } else {
          for (int e = 0; e < lim; ++e) v[e] = src[e];
        }
        if (k >= 0) {
          int a0, a1, c0, c1;
          float fy, fx, m = 0.f;
          bool fresh = true;                                // the pixel changed: its mask is computed once
          for (int e = 0; e < lim; ++e) {
            if (fresh) {
              rise_axis<float>(y, q.up, q.g - 1, a0, a1, fy);
              rise_axis<float>(xx, q.up, q.g - 1, c0, c1, fx);
              m = cam_lerp32(cam_lerp32(nv[a0 * q.g + c0], nv[a0 * q.g + c1], fx), cam_lerp32(nv[a1 * q.g + c0], nv[a1 * q.g + c1], fx), fy);
            }
            const float f = fill[c];
            v[e] = cam_lerp32(f, v[e], m);                   // fill + m (x - fill)
            fresh = false;
            if (++c == q.C) { c = 0; fresh = true; if (++xx == W) { xx = 0; ++y; } }
          }
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

// VEC: L * D % 4 == 0 and 16-byte aligned bases, as occlude_kernel
template <bool VEC>
__global__ __launch_bounds__(256) void feature_ablate_kernel(const float* __restrict__ feat, const int* __restrict__ img_idx,
                                                             const int* __restrict__ kk, float* __restrict__ out, int n, int B,
                                                             int L, int D) {
  const size_t per = (size_t)L * D, groups = (per + 3) / 4, total = (size_t)n * groups;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / groups, gi = idx - rr * groups;
    const int e0 = (int)(4 * gi);
    const int lim = per - e0 < 4 ? (int)(per - e0) : 4;
    float* dst = out + rr * per + e0;
    const int img = img_idx[rr], k = kk[rr];
    float v[4];
    if (img < 0 || img >= B || k < -1 || k >= D) {
      v[0] = v[1] = v[2] = v[3] = sal_nan();
    } else {
      const float* src = feat + (size_t)img * per + e0;
      if (VEC) {
        const float4 t4 = *reinterpret_cast<const float4*>(src);
        v[0] = t4.x; v[1] = t4.y; v[2] = t4.z; v[3] = t4.w;
      } else {
        for (int e = 0; e < lim; ++e) v[e] = src[e];
      }
      int c = e0 % D;
      for (int e = 0; e < lim; ++e) {
        if (c == k) v[e] = 0.f;
        if (++c == D) c = 0;
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int e = 0; e < lim; ++e) dst[e] = v[e];
    }
  }
}

}  // namespace lrp
