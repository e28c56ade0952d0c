// segment_kernels.h — LIME (Ribeiro, Singh & Guestrin, KDD 2016) and KernelSHAP (Lundberg & Lee, NeurIPS 2017) as word
// saliencies: the mask is a binary choice over d segments of the image (a label map from any segmenter), the word scores of the
// masked copies are folded by a weighted linear regression.  The forwards are those of saliency_kernels.h (lrp_encode_images,
// lrp_decoder_forward, lrp_perturb_word_scores); this file holds what is new: the draws, the mask apply, the fit and the gather.
// As there: device pointers, no atomics, every output written by one thread in one fixed order.
//
//  A row's subset is SEG_WORDS = 4 uint32 words: bit j of word j / 32 is segment j, bits at or above d are zero.
//  segment_draws_kernel   one thread per row, Philox4x32-10 of augment_kernels.h under the key (seed low word, seed high word).
//                         Bernoulli (LIME): segment j takes lane j % 4 of counter (j / 4, k, key, 2), on iff (x >> 8) < floor(p 2^24).
//                         Shapley (KernelSHAP): pair q = k >> 1; u = lane 0 of counter (0xFFFFFFFF, q, key, 3); the size is
//                         s = 1 + #{i : u >= thr[i]} over the d - 2 thresholds of the host (the cumulative of the Shapley kernel's
//                         size distribution in 2^-32 units); a partial Fisher-Yates over perm = 0 .. d - 1: for i < s, r = lane
//                         i % 4 of counter (i / 4, q, key, 3), j = i + mulhi32(r, d - i), swap perm[i], perm[j]; the subset is
//                         perm[0 .. s).  An odd k is the complement within d bits of draw k - 1 (antithetic pairs).  The last
//                         counter word keeps the streams apart: 0 the Gaussian augment, 1 RISE, 2 and 3 these.
//  segment_apply_kernel   out = bit(label) ? x : fill[c]: a select, no arithmetic.  An image index outside [0, B) gives a NaN
//                         row, a label outside [0, d) a NaN pixel.
//  segment_fit_kernel     one workgroup per image, everything float64.  Columns u_c(k) of the design matrix, n of them:
//                           LIME form      n = d + 1: u_0 = 1 (the intercept, unpenalised), u_{1 + j} = z_kj
//                           Shapley form   n = d - 1: u_j = z_kj - z_{k, d - 1}, target y_k - z_{k, d - 1} delta
//                         with row weight w_k = wtab[popcount(z_k)] (0 drops the row).  G[a][b] = sum_k w_k u_a u_b (+ ridge on
//                         the penalised diagonal) is kept as a packed lower triangle in LDS, shared by the T words of the image;
//                         every entry is owned by one thread, which adds its K terms in ascending k (u_a u_b is -1, 0 or 1, so
//                         a term is +-w_k exactly): the rows come through LDS in chunks of SEG_CHUNK = 256, which cuts the loop
//                         and not the order.  Right-looking Cholesky in place (column j: pivot, scale, rank-one update of the
//                         trailing triangle, every entry by its one owner); a pivot that is <= 0 or not finite sets status = 1 and
//                         the image's phi and intercept to NaN.  Then per tile of SEG_TT = 8 words (one wave per word): the
//                         right-hand side r[a] = sum_k (w_k y_k) u_a in ascending k, forward and backward substitution column
//                         by column.  Nothing of an image's arithmetic depends on n_img, and nothing of a word's on T.
//  segment_map_kernel     out = (float) phi[t][label], NaN for a label outside [0, d).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "augment_kernels.h"
#include "saliency_kernels.h"

namespace lrp {

constexpr int SEG_MAX_D = 128;
constexpr int SEG_WORDS = 4;
constexpr int SEG_CHUNK = 256;             // rows of the fit staged in LDS at a time
constexpr int SEG_TT = 8;                  // words per pass of the fit's solve: one wave each
constexpr int SEG_FIT_THREADS = 64 * SEG_TT;
constexpr int SEG_DRAW_THREADS = 64;

__device__ __forceinline__ int seg_bit(const unsigned* __restrict__ z, int j) { return (int)((z[j >> 5] >> (j & 31)) & 1u); }

__global__ __launch_bounds__(SEG_DRAW_THREADS) void segment_draws_kernel(const unsigned* __restrict__ key, const int* __restrict__ kk,
                                                                         int n, int d, int shapley, unsigned thresh,
                                                                         const unsigned* __restrict__ thr, unsigned seed_lo,
                                                                         unsigned seed_hi, unsigned* __restrict__ bits) {
  __shared__ unsigned char perm_all[SEG_DRAW_THREADS][SEG_MAX_D];
  unsigned char* perm = perm_all[threadIdx.x];
  for (size_t rr = (size_t)blockIdx.x * SEG_DRAW_THREADS + threadIdx.x; rr < (size_t)n; rr += (size_t)gridDim.x * SEG_DRAW_THREADS) {
    const unsigned k = (unsigned)kk[rr], id = key[rr];
    unsigned z[SEG_WORDS] = {0u, 0u, 0u, 0u};
    if (!shapley) {
      for (int g = 0; 4 * g < d; ++g) {
        const Philox4 r = philox4x32_10((unsigned)g, k, id, 2u, seed_lo, seed_hi);
        for (int e = 0; e < 4 && 4 * g + e < d; ++e)
          if ((r.v[e] >> 8) < thresh) z[(4 * g + e) >> 5] |= 1u << ((4 * g + e) & 31);
      }
    } else {
      const unsigned q = k >> 1;
      const unsigned u = philox4x32_10(0xFFFFFFFFu, q, id, 3u, seed_lo, seed_hi).v[0];
      int s = 1;
      for (int i = 0; i < d - 2; ++i) s += u >= thr[i] ? 1 : 0;
      for (int i = 0; i < d; ++i) perm[i] = (unsigned char)i;
      Philox4 r;
      for (int i = 0; i < s; ++i) {
        if ((i & 3) == 0) r = philox4x32_10((unsigned)(i >> 2), q, id, 3u, seed_lo, seed_hi);
        const int j = i + (int)__umulhi(r.v[i & 3], (unsigned)(d - i));
        const unsigned char a = perm[i], b = perm[j];
        perm[i] = b;
        perm[j] = a;
        z[b >> 5] |= 1u << (b & 31);
      }
      if (k & 1u) {
        for (int w = 0; w < SEG_WORDS; ++w) {
          const int lo = 32 * w;
          const unsigned full = d - lo >= 32 ? 0xFFFFFFFFu : (d > lo ? (1u << (d - lo)) - 1u : 0u);
          z[w] = ~z[w] & full;
        }
      }
    }
    for (int w = 0; w < SEG_WORDS; ++w) bits[rr * SEG_WORDS + w] = z[w];
  }
}

// the groups of four values of saliency_kernels.h's occlude_kernel: VEC under the same condition
template <bool VEC>
__global__ __launch_bounds__(256) void segment_apply_kernel(const float* __restrict__ x, const int* __restrict__ img_idx,
                                                            const unsigned* __restrict__ bits, const int* __restrict__ label,
                                                            const float* __restrict__ fill, float* __restrict__ out, int n, int B,
                                                            int H, int W, int C, int d) {
  const size_t per = (size_t)H * W * C, groups = (per + 3) / 4, total = (size_t)n * groups, hw = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / groups, gi = idx - rr * groups;
    const int e0 = (int)(4 * gi);
    const int lim = per - e0 < 4 ? (int)(per - e0) : 4;
    float* dst = out + rr * per + e0;
    const int img = img_idx[rr];
    float v[4];
    if (img < 0 || img >= B) {
      v[0] = v[1] = v[2] = v[3] = sal_nan();
    } else {
      const float* src = x + (size_t)img * per + e0;
      if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int e = 0; e < lim; ++e) v[e] = src[e];
      }
      const unsigned* z = bits + rr * SEG_WORDS;
      const int* lab = label + (size_t)img * hw;
      int p = e0 / C, c = e0 - p * C;
      int l = lab[p];
      for (int e = 0; e < lim; ++e) {
        if (l < 0 || l >= d) v[e] = sal_nan();
        else if (!seg_bit(z, l)) v[e] = fill[c];
        if (++c == C && e + 1 < lim) { c = 0; l = lab[++p]; }
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int e = 0; e < lim; ++e) dst[e] = v[e];
    }
  }
}

__global__ __launch_bounds__(256) void segment_map_kernel(const double* __restrict__ phi, const int* __restrict__ label,
                                                          float* __restrict__ out, int n_img, int T, int H, int W, int d) {
  const size_t hw = (size_t)H * W, total = (size_t)n_img * T * hw;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t it = idx / hw, p = idx - it * hw, img = it / T;
    const int l = label[img * hw + p];
    out[idx] = (l < 0 || l >= d) ? sal_nan() : (float)phi[it * d + l];
  }
}

// column c of the design matrix at row z (see the header of this file): -1, 0 or 1
__device__ __forceinline__ int seg_feature(const unsigned* __restrict__ z, int c, int shapley, int d) {
  if (shapley) return seg_bit(z, c) - seg_bit(z, d - 1);
  return c == 0 ? 1 : seg_bit(z, c - 1);
}

__device__ __forceinline__ int seg_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // i >= j

// bytes of dynamic LDS: the packed triangle, the right-hand sides of a tile of words, the staged chunk of rows
__host__ __device__ inline size_t segment_fit_lds(int nn) {
  return ((size_t)nn * (nn + 1) / 2 + (size_t)SEG_TT * nn + (size_t)SEG_CHUNK * (1 + SEG_TT)) * sizeof(double) +
         (size_t)SEG_CHUNK * SEG_WORDS * sizeof(unsigned);
}

__global__ __launch_bounds__(SEG_FIT_THREADS) void segment_fit_kernel(const unsigned* __restrict__ bits, const double* __restrict__ wtab,
                                                                      const double* __restrict__ y, const double* __restrict__ delta,
                                                                      double ridge, double* __restrict__ phi, double* __restrict__ icpt,
                                                                      int* __restrict__ status, int K, int T, int d) {
  extern __shared__ double seg_lds[];
  const int shapley = delta != nullptr, nn = shapley ? d - 1 : d + 1, tri = nn * (nn + 1) / 2;
  double* G = seg_lds;                               // [tri]
  double* rhs = G + tri;                             // [SEG_TT][nn]
  double* cw = rhs + SEG_TT * nn;                    // [SEG_CHUNK] row weights
  double* cy = cw + SEG_CHUNK;                       // [SEG_CHUNK][SEG_TT] w_k * target
  unsigned* cz = reinterpret_cast<unsigned*>(cy + SEG_CHUNK * SEG_TT);      // [SEG_CHUNK][SEG_WORDS]
  const int tid = threadIdx.x;
  const size_t img = blockIdx.x;
  const unsigned* zi = bits + img * (size_t)K * SEG_WORDS;
  const double* yi = y + img * (size_t)K * T;
  double* phi_i = phi + img * (size_t)T * d;
  double* icpt_i = icpt + img * (size_t)T;

  // ---- the Gram matrix: every entry by its one owner, rows in ascending k
  for (int e = tid; e < tri; e += SEG_FIT_THREADS) G[e] = 0.0;
  for (int k0 = 0; k0 < K; k0 += SEG_CHUNK) {
    const int rows = min(SEG_CHUNK, K - k0);
    __syncthreads();
    for (int r = tid; r < rows; r += SEG_FIT_THREADS) {
      const unsigned* z = zi + (size_t)(k0 + r) * SEG_WORDS;
      int m = 0;
      for (int w = 0; w < SEG_WORDS; ++w) { cz[r * SEG_WORDS + w] = z[w]; m += __popc(z[w]); }
      cw[r] = m <= d ? wtab[m] : 0.0 / 0.0;         // (bits at or above d: not a row of this problem)
    }
    __syncthreads();
    int i = 0;                                       // the row of entry e: found once per entry
    for (int e = tid; e < tri; e += SEG_FIT_THREADS) {
      while (seg_tri(i + 1, 0) <= e) ++i;
      const int j = e - seg_tri(i, 0);
      double acc = G[e];
      for (int r = 0; r < rows; ++r) {
        const unsigned* z = cz + r * SEG_WORDS;
        const int s = seg_feature(z, i, shapley, d) * seg_feature(z, j, shapley, d);
        const double w = cw[r];
        if (s != 0 && w != 0.0) acc = __dadd_rn(acc, s > 0 ? w : -w);
      }
      G[e] = acc;
    }
  }
  __syncthreads();
  for (int c = tid; c < nn; c += SEG_FIT_THREADS)
    if (shapley || c > 0) G[seg_tri(c, c)] = __dadd_rn(G[seg_tri(c, c)], ridge);
  __syncthreads();

  // ---- Cholesky in place, right-looking
  bool bad = false;
  for (int j = 0; j < nn; ++j) {
    const double piv = G[seg_tri(j, j)];
    if (!(piv > 0.0) || !(piv <= 1.7976931348623157e308)) { bad = true; break; }       // (uniform: every thread reads the same value)
    const double s = sqrt(piv);
    __syncthreads();
    for (int i = j + tid; i < nn; i += SEG_FIT_THREADS) G[seg_tri(i, j)] = i == j ? s : G[seg_tri(i, j)] / s;
    __syncthreads();
    for (int i = j + 1 + tid / 32; i < nn; i += SEG_FIT_THREADS / 32) {
      const double lij = G[seg_tri(i, j)];
      for (int c = j + 1 + (tid & 31); c <= i; c += 32) G[seg_tri(i, c)] = __dsub_rn(G[seg_tri(i, c)], __dmul_rn(lij, G[seg_tri(c, j)]));
    }
    __syncthreads();
  }
  if (tid == 0) status[img] = bad ? 1 : 0;
  if (bad) {
    for (int e = tid; e < T * d; e += SEG_FIT_THREADS) phi_i[e] = 0.0 / 0.0;
    for (int e = tid; e < T; e += SEG_FIT_THREADS) icpt_i[e] = 0.0 / 0.0;
    return;
  }

  // ---- per tile of words: right-hand sides, then L v = r and L^T x = v; wave wv owns word t0 + wv
  const int wv = tid >> 6, lane = tid & 63;
  for (int t0 = 0; t0 < T; t0 += SEG_TT) {
    const int nt = min(SEG_TT, T - t0);
    const int t = t0 + wv;
    double* r_w = rhs + wv * nn;
    double acc[(SEG_MAX_D + 1 + 63) / 64];
#pragma unroll
    for (int m = 0; m < (SEG_MAX_D + 1 + 63) / 64; ++m) acc[m] = 0.0;
    for (int k0 = 0; k0 < K; k0 += SEG_CHUNK) {
      const int rows = min(SEG_CHUNK, K - k0);
      __syncthreads();
      for (int r = tid; r < rows; r += SEG_FIT_THREADS) {
        const unsigned* z = zi + (size_t)(k0 + r) * SEG_WORDS;
        int m = 0;
        for (int w = 0; w < SEG_WORDS; ++w) { cz[r * SEG_WORDS + w] = z[w]; m += __popc(z[w]); }
        const double w = m <= d ? wtab[m] : 0.0 / 0.0;
        const int zl = shapley ? seg_bit(z, d - 1) : 0;
        for (int q = 0; q < nt; ++q) {
          double v = yi[(size_t)(k0 + r) * T + t0 + q];
          if (zl) v = __dsub_rn(v, delta[img * (size_t)T + t0 + q]);
          cy[r * SEG_TT + q] = w != 0.0 ? __dmul_rn(w, v) : 0.0;
        }
      }
      __syncthreads();
      if (wv < nt) {
#pragma unroll
        for (int m = 0; m < (SEG_MAX_D + 1 + 63) / 64; ++m) {
          const int a = lane + 64 * m;
          if (a < nn) {
            double s = acc[m];
            for (int r = 0; r < rows; ++r) {
              const int u = seg_feature(cz + r * SEG_WORDS, a, shapley, d);
              const double v = cy[r * SEG_TT + wv];
              if (u != 0) s = __dadd_rn(s, u > 0 ? v : -v);
            }
            acc[m] = s;
          }
        }
      }
    }
    if (wv < nt) {
#pragma unroll
      for (int m = 0; m < (SEG_MAX_D + 1 + 63) / 64; ++m)
        if (lane + 64 * m < nn) r_w[lane + 64 * m] = acc[m];
    }
    __syncthreads();
    // (a wave past the tile's last word carries zeros through the same barriers)
    for (int j = 0; j < nn; ++j) {                   // forward: v_j = r_j / L_jj, r_i -= L_ij v_j below it
      const double vj = wv < nt ? r_w[j] / G[seg_tri(j, j)] : 0.0;
      __syncthreads();
      if (wv < nt) {
        if (lane == 0) r_w[j] = vj;
        for (int i = j + 1 + lane; i < nn; i += 64) r_w[i] = __dsub_rn(r_w[i], __dmul_rn(G[seg_tri(i, j)], vj));
      }
      __syncthreads();
    }
    for (int j = nn - 1; j >= 0; --j) {              // backward: x_j = v_j / L_jj, v_i -= L_ji x_j above it
      const double xj = wv < nt ? r_w[j] / G[seg_tri(j, j)] : 0.0;
      __syncthreads();
      if (wv < nt) {
        if (lane == 0) r_w[j] = xj;
        for (int i = lane; i < j; i += 64) r_w[i] = __dsub_rn(r_w[i], __dmul_rn(G[seg_tri(j, i)], xj));
      }
      __syncthreads();
    }
    if (wv < nt) {
      double* out = phi_i + (size_t)t * d;
      if (shapley) {
        for (int c = lane; c < d - 1; c += 64) out[c] = r_w[c];
        if (lane == 0) {
          double last = delta[img * (size_t)T + t];
          for (int c = 0; c < d - 1; ++c) last = __dsub_rn(last, r_w[c]);
          out[d - 1] = last;
          icpt_i[t] = 0.0;
        }
      } else {
        for (int c = lane; c < d; c += 64) out[c] = r_w[1 + c];
        if (lane == 0) icpt_i[t] = r_w[0];
      }
    }
  }
}

}  // namespace lrp
