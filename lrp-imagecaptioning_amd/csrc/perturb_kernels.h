// perturb_kernels.h — perturbation ("pixel-flipping") analysis (the reference's innvestigate/tools/perturbate.py, cited
// PT:): rank the regions of a heat-map by relevance, replace the top-k regions of the image, read the explained word's
// score off the logits of the forward that follows.  Three launches, one workgroup per (image, word) unit, fixed-order fp64
// reductions and no atomics: a unit's results do not depend on what else shares the launch.
//
//  perturb_rank_kernel        (n, H, W, C) heat-maps (float32 / float64) -> (n, nreg) int32 ranks (+ the fp64 scores).
//      PT:167 reduce over channels, PT:105-116 reflect padding (by index arithmetic: nothing padded is stored), PT:125-128
//      aggregate over a region, PT:79-84 ranks.  One thread owns a region and adds its pixels in raster order (each pixel
//      its channels in order), so the score is one fixed sequence of fp64 operations a host loop can repeat bit for bit.
//      rank[i] = #{j : s_j > s_i or (s_j == s_i and j < i)}: counted over the scores in LDS (every lane reads the same
//      s_j: a broadcast).  NaN scores rank last, among themselves by index.
//  perturb_apply_kernel       x (B, H, W, C) gathered by img_idx -> (n, H, W, C) with the regions of rank <= k - 1
//      replaced (PT:74-76, PT:130-148), channel 0 only or every channel.  The clip of PT:142-146 acts on the whole unit as
//      soon as one region is perturbed, and in the reference every later region is computed from the clipped tensor: here
//      the unit is clipped first, perturbed, and clipped again.  'mean' gets a second pass: one thread per perturbed
//      (region, channel) adds the padded region in raster order in fp64, rounds once and fills the region.
//  perturb_word_score_kernel  logits (B, Tm, V) float64 -> per unit l[k] and l[k] - (max + log sum exp(l - max)) of row t - 1.
#pragma once
#include <hip/hip_runtime.h>
#include "decoder_kernels.h"
#include "eval_kernels.h"

namespace lrp {

constexpr int PERTURB_MAX_REGIONS = 4096;
enum { PERTURB_FN_MEAN = 0, PERTURB_FN_MAX = 1 };                                   // reduce / aggregate
enum { PERTURB_ZEROS = 0, PERTURB_MEAN = 1, PERTURB_INVERT = 2, PERTURB_NOISE = 3 };  // perturbation function

struct PerturbGeom {
  int H, W, C;        // one map / image
  int rh, rw;         // region shape
  int Hr, Wr;         // regions per column / row of the padded map
  int bh, bw;         // padding before (rows, columns); the rest of the padding comes after
};

// np.pad(mode='reflect'): index i of an axis of length n, mirrored about the edge samples (the edge is not repeated)
__device__ __forceinline__ int perturb_mirror(int i, int n) {
  if (n == 1) return 0;
  const int per = 2 * (n - 1);
  i %= per;
  if (i < 0) i += per;
  return i >= n ? per - i : i;
}

__device__ __forceinline__ double perturb_max(double a, double b) {       // np.maximum: NaN propagates
  return a != a ? a : (b != b ? b : (a > b ? a : b));
}

template <typename T>
__global__ __launch_bounds__(256) void perturb_rank_kernel(const T* __restrict__ Rall, PerturbGeom g, int reduce, int aggregate,
                                                           double sign, int* __restrict__ ranks, double* __restrict__ scores) {
  extern __shared__ double sc[];                            // nreg scores
  const int tid = threadIdx.x, nreg = g.Hr * g.Wr;
  const T* R = Rall + (size_t)blockIdx.x * g.H * g.W * g.C;
  for (int r = tid; r < nreg; r += 256) {
    const int ry = r / g.Wr, rx = r - ry * g.Wr;
    double acc = 0.0;
    for (int dy = 0; dy < g.rh; ++dy) {
      const int y = perturb_mirror(ry * g.rh + dy - g.bh, g.H);
      for (int dx = 0; dx < g.rw; ++dx) {
        const int x = perturb_mirror(rx * g.rw + dx - g.bw, g.W);
        const T* p = R + ((size_t)y * g.W + x) * g.C;
        double v = (double)p[0];
        for (int c = 1; c < g.C; ++c) v = reduce == PERTURB_FN_MEAN ? v + (double)p[c] : perturb_max(v, (double)p[c]);
        if (reduce == PERTURB_FN_MEAN) v = v / (double)g.C;
        acc = (dy | dx) == 0 ? v : (aggregate == PERTURB_FN_MEAN ? acc + v : perturb_max(acc, v));
      }
    }
    if (aggregate == PERTURB_FN_MEAN) acc = acc / (double)(g.rh * g.rw);
    acc = sign * acc;
    sc[r] = acc;
    if (scores) scores[(size_t)blockIdx.x * nreg + r] = acc;
  }
  __syncthreads();
  for (int i = tid; i < nreg; i += 256) {
    const double si = sc[i];
    const bool nan_i = si != si;
    int cnt = 0;
    for (int j = 0; j < nreg; ++j) {
      const double sj = sc[j];
      const bool before = nan_i ? (sj == sj || j < i) : (sj > si || (sj == si && j < i));
      cnt += before ? 1 : 0;
    }
    ranks[(size_t)blockIdx.x * nreg + i] = cnt;
  }
}

__device__ __forceinline__ float perturb_clip(float v, float lo, float hi) {    // np.clip: NaN stays NaN
  return v < lo ? lo : (v > hi ? hi : v);
}

__global__ __launch_bounds__(256) void perturb_apply_kernel(const float* __restrict__ x, const int* __restrict__ img_idx,
                                                            const int* __restrict__ ranks, const double* __restrict__ kk,
                                                            const float* __restrict__ noise, float* __restrict__ out, int B,
                                                            PerturbGeom g, int mode, int all_channels, int has_range, float lo,
                                                            float hi) {
  __shared__ unsigned char pert[PERTURB_MAX_REGIONS];
  const int tid = threadIdx.x, u = blockIdx.x, nreg = g.Hr * g.Wr, nval = g.H * g.W * g.C;
  float* o = out + (size_t)u * nval;
  const int img = img_idx[u];
  if (img < 0 || img >= B) {                                // (the whole workgroup takes this branch: no barrier is skipped)
    for (int i = tid; i < nval; i += 256) o[i] = __int_as_float(0x7fc00000);
    return;
  }
  const float* xi = x + (size_t)img * nval;
  const double k = kk[u];
  const bool clip = has_range && k >= 1.0;
  for (int r = tid; r < nreg; r += 256) pert[r] = (double)ranks[(size_t)u * nreg + r] <= k - 1.0 ? 1 : 0;
  __syncthreads();
  for (int i = tid; i < nval; i += 256) {
    const int p = i / g.C, c = i - p * g.C, y = p / g.W, xx = p - y * g.W;
    float v = xi[i];
    if (clip) v = perturb_clip(v, lo, hi);
    const int r = ((y + g.bh) / g.rh) * g.Wr + (xx + g.bw) / g.rw;
    if (pert[r] && (all_channels || c == 0)) {
      if (mode == PERTURB_MEAN) continue;                   // the second pass writes this value
      v = mode == PERTURB_ZEROS ? 0.0f : (mode == PERTURB_INVERT ? -v : noise[(size_t)u * nval + i]);
      if (clip) v = perturb_clip(v, lo, hi);
    }
    o[i] = v;
  }
  if (mode != PERTURB_MEAN) return;
  const int nc = all_channels ? g.C : 1;
  for (int task = tid; task < nreg * nc; task += 256) {
    const int r = task / nc, c = task - r * nc;
    if (!pert[r]) continue;
    const int ry = r / g.Wr, rx = r - ry * g.Wr;
    double acc = 0.0;
    for (int dy = 0; dy < g.rh; ++dy) {
      const int y = perturb_mirror(ry * g.rh + dy - g.bh, g.H);
      for (int dx = 0; dx < g.rw; ++dx) {
        const int xx = perturb_mirror(rx * g.rw + dx - g.bw, g.W);
        float v = xi[((size_t)y * g.W + xx) * g.C + c];
        if (clip) v = perturb_clip(v, lo, hi);
        acc = (dy | dx) == 0 ? (double)v : acc + (double)v;
      }
    }
    float m = (float)(acc / (double)(g.rh * g.rw));
    if (clip) m = perturb_clip(m, lo, hi);
    for (int dy = 0; dy < g.rh; ++dy) {
      const int y = ry * g.rh + dy - g.bh;
      if (y < 0 || y >= g.H) continue;
      for (int dx = 0; dx < g.rw; ++dx) {
        const int xx = rx * g.rw + dx - g.bw;
        if (xx < 0 || xx >= g.W) continue;
        o[((size_t)y * g.W + xx) * g.C + c] = m;
      }
    }
  }
}

// One workgroup per unit: row t - 1 of image slot `slot`, column `col`.  A unit outside the logits reads nothing: NaN.
__global__ __launch_bounds__(256) void perturb_word_score_kernel(const double* __restrict__ preds, const int* __restrict__ slot,
                                                                 const int* __restrict__ t, const int* __restrict__ col, int B,
                                                                 int Tm, int V, double* __restrict__ logit,
                                                                 double* __restrict__ logp) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
  const int s = slot[u], tt = t[u], k = col[u];
  if (s < 0 || s >= B || tt < 1 || tt > Tm || k < 0 || k >= V) {
    if (tid == 0) logit[u] = logp[u] = 0.0 / 0.0;
    return;
  }
  const double* l = preds + ((size_t)s * Tm + (tt - 1)) * V;
  double mx = -INFINITY;
  for (int i = tid; i < V; i += 256) mx = fmax(mx, l[i]);
  mx = eval_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  double sum = 0.0;
  for (int i = tid; i < V; i += 256) sum += exp(l[i] - mx);
  sum = wave_sum_d(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    sum = ((red[0] + red[1]) + red[2]) + red[3];
    logit[u] = l[k];
    logp[u] = l[k] - (mx + log(sum));
  }
}

}  // namespace lrp
