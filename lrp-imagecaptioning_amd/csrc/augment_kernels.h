// augment_kernels.h — augment and reduce of the reference's AugmentReduceBase wrappers (innvestigate/analyzer/wrapper.py:78-345:
// GaussianSmoother behind SmoothGrad, PathIntegrator behind IntegratedGradients) as streaming kernels in the style of
// eval_kernels.h: device pointers, no atomics, every output element written by exactly one thread in a fixed order, so a
// result never depends on how the sample rows were cut into chunks.
//
//  Sample matrix: (B * n, per_image) in np.repeat order (wrapper.py:169): row r = b * n + s is sample s of image b.
//  augment_gaussian_kernel   row r, element i:  x[b][i] + sigma * N(seed, r, i)
//      N: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 /
//      0xBB67AE85), key = (seed low word, seed high word), counter = (g low word, g high word, r, 0) with g = i / 4.  The
//      four outputs x0..x3 make two Box-Muller pairs: u = ((x >> 8) + 0.5) 2^-24 in (0, 1),
//      z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1), (z2, z3) from (u2, u3) alike: element i takes
//      z[i % 4].  |z| <= sqrt(-2 ln 2^-25) = 5.89.  u has 25 significant bits; ln u and the angle are evaluated on exactly
//      representable arguments (ln u = log1p(-(1 - u)) and the angle reduced by one turn in the upper half of the range), with
//      the precise logf / log1pf / sincospif: no fast-math intrinsic.
//  augment_path_kernel       mode 0: x + (s / n) (x - ref)   (what wrapper.py:268-288 computes: away from the reference)
//                            mode 1: ref + (s / n) (x - ref) (the published straight path); each operation rounded on its
//                            own in float32, as numpy does.  ref: one scalar, or a (B, per_image) tensor.
//  reduce_accum_kernel       acc[b][i] += sum over the chunk's rows of image b, ascending s, of post(map[r][i]) in fp64;
//                            post = none / |.| / square (gradient_based.py:110-137 post-processes each sample, then the mean)
//  reduce_finish_kernel      out[b][i] = float(acc / n [* (x - ref)])  (wrapper.py:171-174, :290-296), rounded once
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lrp {

enum { AUG_POST_NONE = 0, AUG_POST_ABS = 1, AUG_POST_SQUARE = 2 };

struct Philox4 { unsigned v[4]; };

__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// one Box-Muller pair from two Philox words (see the header of this file)
__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& z0, float& z1) {
  const unsigned ka = xa >> 8, kb = xb >> 8;
  float ln_u;
  if (ka < (1u << 23)) ln_u = logf(((float)ka + 0.5f) * 0x1p-24f);
  else ln_u = log1pf(-(((float)(0xFFFFFFu - ka) + 0.5f) * 0x1p-24f));
  const float turn2 = kb < (1u << 23) ? ((float)kb + 0.5f) * 0x1p-23f : -(((float)(0xFFFFFFu - kb) + 0.5f) * 0x1p-23f);
  float sn, cs;
  sincospif(turn2, &sn, &cs);
  const float rad = sqrtf(-2.f * ln_u);
  z0 = rad * cs; z1 = rad * sn;
}

__global__ __launch_bounds__(256) void augment_gaussian_kernel(const float* __restrict__ x, float* __restrict__ out, int n,
                                                               size_t per_image, int r0, int count, float sigma,
                                                               unsigned seed_lo, unsigned seed_hi) {
  const size_t groups = (per_image + 3) / 4, total = (size_t)count * groups;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / groups, g = idx - rr * groups;
    const unsigned r = (unsigned)r0 + (unsigned)rr;
    const size_t b = r / (unsigned)n;
    const Philox4 p = philox4x32_10((unsigned)g, (unsigned)((unsigned long long)g >> 32), r, 0u, seed_lo, seed_hi);
    float z[4];
    box_muller(p.v[0], p.v[1], z[0], z[1]);
    box_muller(p.v[2], p.v[3], z[2], z[3]);
    const float* src = x + b * per_image + 4 * g;
    float* dst = out + rr * per_image + 4 * g;
    const int lim = per_image - 4 * g < 4 ? (int)(per_image - 4 * g) : 4;     // a tail group writes fewer than four values
    for (int e = 0; e < lim; ++e) dst[e] = __fadd_rn(src[e], __fmul_rn(sigma, z[e]));
  }
}

// ref_t != nullptr: the (B, per_image) reference tensor; otherwise the scalar ref_s
__global__ __launch_bounds__(256) void augment_path_kernel(const float* __restrict__ x, const float* __restrict__ ref_t, float ref_s,
                                                           float* __restrict__ out, int n, size_t per_image, int r0, int count,
                                                           int mode) {
  const size_t total = (size_t)count * per_image;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / per_image, i = idx - rr * per_image;
    const unsigned r = (unsigned)r0 + (unsigned)rr;
    const size_t b = r / (unsigned)n;
    const float alpha = __fdiv_rn((float)(r - (unsigned)b * (unsigned)n), (float)n);
    const float xv = x[b * per_image + i], rv = ref_t ? ref_t[b * per_image + i] : ref_s;
    const float step = __fmul_rn(alpha, __fsub_rn(xv, rv));
    out[idx] = __fadd_rn(mode == 0 ? xv : rv, step);
  }
}

// one thread per (image, element) of the images the chunk [r0, r0 + count) touches; maps: (count, per_image), row 0 = sample r0
__global__ __launch_bounds__(256) void reduce_accum_kernel(const float* __restrict__ maps, double* __restrict__ acc, int n,
                                                           size_t per_image, int r0, int count, int post) {
  const int b_lo = r0 / n, b_hi = (r0 + count - 1) / n;
  const size_t total = (size_t)(b_hi - b_lo + 1) * per_image;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t bb = idx / per_image, i = idx - bb * per_image;
    const int b = b_lo + (int)bb;
    const int lo = b * n > r0 ? b * n : r0, hi = (b + 1) * n < r0 + count ? (b + 1) * n : r0 + count;
    double a = acc[(size_t)b * per_image + i];
    for (int r = lo; r < hi; ++r) {
      const double v = (double)maps[(size_t)(r - r0) * per_image + i];
      a += post == AUG_POST_ABS ? fabs(v) : post == AUG_POST_SQUARE ? v * v : v;
    }
    acc[(size_t)b * per_image + i] = a;
  }
}

// has_factor: out = acc / n * (x - ref) (PathIntegrator); x, ref_t / ref_s as in augment_path_kernel
__global__ __launch_bounds__(256) void reduce_finish_kernel(const double* __restrict__ acc, float* __restrict__ out, int n, size_t total,
                                                            int has_factor, const float* __restrict__ x,
                                                            const float* __restrict__ ref_t, float ref_s) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    double v = acc[idx] / (double)n;
    if (has_factor) v *= (double)x[idx] - (double)(ref_t ? ref_t[idx] : ref_s);
    out[idx] = (float)v;
  }
}

}  // namespace lrp
