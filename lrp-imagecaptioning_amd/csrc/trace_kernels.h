// trace_kernels.h — per-layer relevance of the VGG-style LRP walk (Encoder::explain_traced): the reversed tensors of
// innvestigate's reverse_keep_tensors / reverse_check_min_max_values / reverse_check_finite (analyzer/base.py:570-603, :769-802).
//
// The walk carries S_l = R_l / den_l, never R_l.  The traced walk runs layer l's transposed conv with a plain fp32 accumulator out
// (acc = convT(S_l), no gate in the epilogue) and trace_layer_kernel behind it:
//   R at the input of conv l        = a_{l-1} * acc          (a_{l-1}: the kept layer input, post-ReLU / the pooled activation)
//   R at the input of a 2x2 pool    = that value at the forward's arg-max cell (first in scan order), exact 0.0 at the other three
//   S_{l-1}                         = gate_{l-1} * acc        (one or two chains, fp32 or split8, where the next conv reads it)
// and the four statistics of both tensors per heat-map row: minimum, maximum, sum (float64) and the count of inf / NaN, made from the
// very fp32 values the keep buffer holds.
//
// Order of every reduction: a row's items are cut into chunks of TRACE_ITEMS_PER_BLOCK, one block per chunk; a thread adds its
// items in ascending order, the wave folds with a xor butterfly (both partners add the same two numbers: one result), thread 0
// folds the waves in wave order, trace_finish_kernel folds a row's chunks in chunk order.  Nothing depends on the row count of the
// call or on another row; there is no atomic.
#pragma once
#include "cnn_kernels.h"
#include "common.h"

namespace lrp {

constexpr int TRACE_ITEMS_PER_THREAD = 8;
constexpr int TRACE_ITEMS_PER_BLOCK = 256 * TRACE_ITEMS_PER_THREAD;
constexpr int TRACE_PART = 5;                            // doubles per partial: min, max, sum, non-finite count, NaN count

// Running statistics of one tensor row.  Minimum and maximum order -0.0 below +0.0 and skip NaN; a NaN anywhere makes both NaN
// at the end (numpy's min / max).  The counts are doubles: exact below 2^53.
struct TraceAcc {
  float mn, mx;
  double sum, nonfinite, nan;
};
__device__ inline TraceAcc trace_acc_empty() { return TraceAcc{__builtin_inff(), -__builtin_inff(), 0.0, 0.0, 0.0}; }
__device__ inline bool trace_below(float a, float b) {
  return a < b || (a == b && (__float_as_uint(a) >> 31) > (__float_as_uint(b) >> 31));
}
__device__ inline void trace_acc_add(TraceAcc& s, float v) {
  const unsigned u = __float_as_uint(v);
  s.sum += (double)v;
  if ((u & 0x7f800000u) == 0x7f800000u) {
    s.nonfinite += 1.0;
    if (u & 0x007fffffu) { s.nan += 1.0; return; }
  }
  if (trace_below(v, s.mn)) s.mn = v;
  if (trace_below(s.mx, v)) s.mx = v;
}
__device__ inline void trace_acc_merge(TraceAcc& s, const TraceAcc& o) {
  if (trace_below(o.mn, s.mn)) s.mn = o.mn;
  if (trace_below(s.mx, o.mx)) s.mx = o.mx;
  s.sum += o.sum; s.nonfinite += o.nonfinite; s.nan += o.nan;
}
// block of NT threads (a multiple of 64) -> the block's statistics in thread 0; lds: NT / 64 entries
template <int NT>
__device__ inline TraceAcc trace_block_reduce(TraceAcc s, TraceAcc* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    TraceAcc p;
    p.mn = __shfl_xor(s.mn, o); p.mx = __shfl_xor(s.mx, o);
    p.sum = __shfl_xor(s.sum, o); p.nonfinite = __shfl_xor(s.nonfinite, o); p.nan = __shfl_xor(s.nan, o);
    trace_acc_merge(s, p);
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NT / 64; ++w) trace_acc_merge(s, lds[w]);
  return s;
}
__device__ inline void trace_store_partial(double* p, const TraceAcc& s) {
  p[0] = s.mn; p[1] = s.mx; p[2] = s.sum; p[3] = s.nonfinite; p[4] = s.nan;
}
__device__ inline void trace_store_stats(double* st, double mn, double mx, double sum, double nonfinite, double nan) {
  const double q = __builtin_nan("");
  st[0] = nan > 0.0 ? q : mn; st[1] = nan > 0.0 ? q : mx; st[2] = sum; st[3] = nonfinite;
}

// lrp_op_tensor_stats: x (rows, per_row) fp32 -> stats (rows, 4) float64.  One block of 1024 threads per row (an operator on
// caller-owned buffers has no scratch for partials): thread t adds elements t, t + 1024, ... in that order.
__global__ __launch_bounds__(1024) void tensor_stats_kernel(const float* __restrict__ x, size_t per_row, double* __restrict__ stats) {
  __shared__ TraceAcc lds[1024 / 64];
  const float* r = x + (size_t)blockIdx.x * per_row;
  TraceAcc s = trace_acc_empty();
  for (size_t i = threadIdx.x; i < per_row; i += 1024) trace_acc_add(s, r[i]);
  s = trace_block_reduce<1024>(s, lds);
  if (threadIdx.x == 0) trace_store_stats(stats + (size_t)blockIdx.x * 4, s.mn, s.mx, s.sum, s.nonfinite, s.nan);
}

struct TraceLayerArgs {
  const float* acc;      // (n, H, W, C) fp32: convT(S_l) through conv l, no gate
  const float* a;        // (images, H, W, C): the kept input of conv l
  const float* gpos;     // POOL: (images, 2H, 2W, C) the forward's gate G+ of the pooled layer below — its arg-max mask
  const float* g0;       // gates of the layer below, one per chain it walks with: (images, Hf, Wf, C), Hf = 2H behind a pool
  const float* g1;
  const int* row2img;
  float* S;              // (n, Hf, Wf, K C): [chain 0 (C) | chain 1 (C)] per pixel, fp32 or split8
  float* keep_conv;      // (n, H, W, C) or nullptr: R at the input of conv l
  float* keep_pool;      // POOL: (n, 2H, 2W, C) or nullptr: R at the input of the pool
  double* part_conv;     // partials [n][nblk][TRACE_PART] of the two tensors
  double* part_pool;
  int n, H, W, C;
};

// grid (nblk, n); an item is one pixel of conv l's input x G channels (G = 8 with split8 output, 4 otherwise)
template <bool POOL, bool SPLIT, int K>
__global__ __launch_bounds__(256) void trace_layer_kernel(TraceLayerArgs t) {
  constexpr int G = SPLIT ? 8 : 4;
  __shared__ TraceAcc lds[256 / 64];
  const int row = blockIdx.y, img = t.row2img ? t.row2img[row] : row;
  const int cg = t.C / G;
  const size_t items = (size_t)t.H * t.W * cg;
  const int Hf = POOL ? 2 * t.H : t.H, Wf = POOL ? 2 * t.W : t.W;
  TraceAcc sc = trace_acc_empty(), sp = trace_acc_empty();
  for (int j = 0; j < TRACE_ITEMS_PER_THREAD; ++j) {
    const size_t it = (size_t)blockIdx.x * TRACE_ITEMS_PER_BLOCK + (size_t)j * 256 + threadIdx.x;
    if (it >= items) break;
    const size_t pix = it / cg;
    const int c = (int)(it - pix * cg) * G, y = (int)(pix / t.W), x = (int)(pix - (size_t)y * t.W);
    const size_t po = (size_t)y * t.W + x, HW = (size_t)t.H * t.W;
    float acc[G], av[G], R[G];
#pragma unroll
    for (int q = 0; q < G; q += 4) {
      *reinterpret_cast<f32x4*>(acc + q) = *reinterpret_cast<const f32x4*>(t.acc + ((size_t)row * HW + po) * t.C + c + q);
      *reinterpret_cast<f32x4*>(av + q) = *reinterpret_cast<const f32x4*>(t.a + ((size_t)img * HW + po) * t.C + c + q);
    }
#pragma unroll
    for (int q = 0; q < G; ++q) {
      R[q] = av[q] * acc[q];
      trace_acc_add(sc, R[q]);
    }
    if (t.keep_conv) {
#pragma unroll
      for (int q = 0; q < G; q += 4)
        *reinterpret_cast<f32x4*>(t.keep_conv + ((size_t)row * HW + po) * t.C + c + q) = *reinterpret_cast<const f32x4*>(R + q);
    }
    auto put_S = [&](size_t fpix_row, const float* s, int k) {    // chain k of full-resolution pixel fpix_row (row-relative index folded in)
      float* d = t.S + fpix_row * (size_t)(K * t.C) + (size_t)k * t.C + c;
      if constexpr (SPLIT) {
        split8_store(s, d);
      } else {
        *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(s);
      }
    };
    if constexpr (!POOL) {
      const size_t go = ((size_t)img * HW + po) * t.C + c;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float* g = k ? t.g1 : t.g0;
        float gv[G], s[G];
#pragma unroll
        for (int q = 0; q < G; q += 4) *reinterpret_cast<f32x4*>(gv + q) = *reinterpret_cast<const f32x4*>(g + go + q);
#pragma unroll
        for (int q = 0; q < G; ++q) s[q] = gv[q] * acc[q];
        put_S((size_t)row * HW + po, s, k);
      }
    } else {
      size_t cell[4];
      int arg[G];
#pragma unroll
      for (int q = 0; q < G; ++q) arg[q] = 0;
#pragma unroll
      for (int p = 3; p >= 0; --p) {                     // the one cell with G+ != 0; a window of zeros: the first in scan order
        cell[p] = (size_t)(2 * y + (p >> 1)) * Wf + 2 * x + (p & 1);
        float gp[G];
#pragma unroll
        for (int q = 0; q < G; q += 4)
          *reinterpret_cast<f32x4*>(gp + q) = *reinterpret_cast<const f32x4*>(t.gpos + ((size_t)img * Hf * Wf + cell[p]) * t.C + c + q);
#pragma unroll
        for (int q = 0; q < G; ++q)
          if (gp[q] != 0.f) arg[q] = p;
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float Rp[G];
#pragma unroll
        for (int q = 0; q < G; ++q) {
          Rp[q] = arg[q] == p ? R[q] : 0.f;
          trace_acc_add(sp, Rp[q]);
        }
        const size_t fo = (size_t)row * Hf * Wf + cell[p];
        if (t.keep_pool) {
#pragma unroll
          for (int q = 0; q < G; q += 4) *reinterpret_cast<f32x4*>(t.keep_pool + fo * t.C + c + q) = *reinterpret_cast<const f32x4*>(Rp + q);
        }
        const size_t go = ((size_t)img * Hf * Wf + cell[p]) * t.C + c;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float* g = k ? t.g1 : t.g0;
          float gv[G], s[G];
#pragma unroll
          for (int q = 0; q < G; q += 4) *reinterpret_cast<f32x4*>(gv + q) = *reinterpret_cast<const f32x4*>(g + go + q);
#pragma unroll
          for (int q = 0; q < G; ++q) s[q] = arg[q] == p ? gv[q] * acc[q] : 0.f;
          put_S(fo, s, k);
        }
      }
    }
  }
  const size_t pi = ((size_t)row * gridDim.x + blockIdx.x) * TRACE_PART;
  sc = trace_block_reduce<256>(sc, lds);
  if (threadIdx.x == 0) trace_store_partial(t.part_conv + pi, sc);
  if constexpr (POOL) {
    __syncthreads();                                     // (lds is reused)
    sp = trace_block_reduce<256>(sp, lds);
    if (threadIdx.x == 0) trace_store_partial(t.part_pool + pi, sp);
  }
}

// a row's partials, in chunk order -> its four statistics; one thread per row
__global__ __launch_bounds__(64) void trace_finish_kernel(const double* __restrict__ part, int n, int nblk, double* __restrict__ stats) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  const double* p = part + (size_t)row * nblk * TRACE_PART;
  double mn = p[0], mx = p[1], sum = p[2], nf = p[3], nan = p[4];
  for (int b = 1; b < nblk; ++b) {
    const double* q = p + (size_t)b * TRACE_PART;
    // (the partials' minima and maxima are floats widened: the sign of a zero decides a tie as in trace_below)
    if (trace_below((float)q[0], (float)mn)) mn = q[0];
    if (trace_below((float)mx, (float)q[1])) mx = q[1];
    sum += q[2]; nf += q[3]; nan += q[4];
  }
  trace_store_stats(stats + (size_t)row * 4, mn, mx, sum, nf, nan);
}

}  // namespace lrp
