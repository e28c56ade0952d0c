// decoder_gridtd_kernels.h — grid-TD (bottom-up / top-down) decoder, E:995-1321.
//   forward replay   _forward_beam_search                 E:1092-1178
//   per-token LRP    _explain_lstm_single_word_sequence   E:1180-1321
// In the reference this decoder runs in float64 from the first step on (x2t is float64 because
// context_hat is, and np.vstack then promotes every state array), so everything here is double.
// Reference quirks reproduced on purpose: logits are cached from h2 alone (E:1154) while the
// output rule is fed h2 + c_hat (E:1212-1217); relevance routing uses '+=' (E:1252-1254, :1288,
// :1300); r_V is a float32 accumulator that is rounded after every step's '+=' (E:1189, :1293);
// r_words is not normalised (E:1320).
#pragma once
#include <hip/hip_runtime.h>
#include "decoder_kernels.h"

namespace lrp {

__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }

// xh1[b] = [ h2_{i} | relu(glob_pre) | emb(tok) | h1_{i} ]  (E:1131-1136) and x1t[b][i] = first H+2E
__global__ __launch_bounds__(256) void gtd_prep_x1_kernel(const float* __restrict__ emb, const float* __restrict__ glob_pre,
                                                          const double* __restrict__ h1t, const double* __restrict__ h2t,
                                                          const int* __restrict__ cap, double* __restrict__ xh1,
                                                          double* __restrict__ x1t, int step, int Tm, int E, int H, int V,
                                                          int sos) {
  const int b = blockIdx.x, S = Tm + 1;
  int tok = (step == 0 ? sos : cap[b * Tm + step - 1]) - 1;
  tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
  const int K1 = H + 2 * E, Nd = K1 + H;
  for (int e = threadIdx.x; e < Nd; e += 256) {
    double v;
    if (e < H) v = h2t[((size_t)b * S + step) * H + e];
    else if (e < H + E) v = (double)fmaxf(glob_pre[(size_t)b * E + e - H], 0.f);
    else if (e < K1) v = (double)emb[(size_t)tok * E + e - H - E];
    else v = h1t[((size_t)b * S + step) * H + e - K1];
    xh1[(size_t)b * Nd + e] = v;
    if (e < K1) x1t[((size_t)b * Tm + step) * K1 + e] = v;
  }
}

// LSTM pointwise (E:129-138), optionally with the sentinel s = tanh(c) * sigmoid(gate)  (E:1145)
// z arrives as `ks` split-K slabs (`slab` doubles apart), added here in a fixed order
__global__ __launch_bounds__(256) void gtd_pointwise_kernel(const double* __restrict__ z, int ldz, int ks, size_t slab,
                                                            double* __restrict__ ht,
                                                            double* __restrict__ ct, double* __restrict__ gt,
                                                            double* __restrict__ it, double* __restrict__ ft,
                                                            double* __restrict__ st, double* __restrict__ hu,
                                                            double* __restrict__ ot, int step, int Tm, int H) {
  const int b = blockIdx.x, S = Tm + 1;
  const double* zb = z + (size_t)b * ldz;
  const size_t prev = ((size_t)b * S + step) * H, cur = prev + H;
  for (int j = threadIdx.x; j < H; j += 256) {
    double zz[5];
    const int ng = st ? 5 : 4;
    for (int g = 0; g < ng; ++g) {
      double v = zb[g * H + j];
      for (int q = 1; q < ks; ++q) v += zb[(size_t)q * slab + g * H + j];
      zz[g] = v;
    }
    const double i_ = sigmoid_d(zz[0]), f_ = sigmoid_d(zz[1]), g_ = zz[2], o_ = sigmoid_d(zz[3]);
    const double c = f_ * ct[prev + j] + i_ * tanh(g_);
    const double tc = tanh(c);
    const double h = o_ * tc;
    ht[cur + j] = h;
    ct[cur + j] = c;
    gt[cur + j] = g_;
    it[cur + j] = i_;
    ft[cur + j] = f_;
    ot[cur + j] = o_;                                  // (gradient baselines, E:1327-1342)
    if (st) st[cur + j] = tc * sigmoid_d(zz[4]);
    if (hu) hu[((size_t)b * Tm + step) * H + j] = h;          // rows of the output-layer GEMM (h2 only, E:1154)
  }
}

// attention + sentinel mix on h1 (E:1140-1149), then xh2[b] = [ c_hat | h1 | h2_{i} ] and x2t (E:1151)
// dynamic LDS: double hp[H], sp[H], pre[L+1]
__global__ __launch_bounds__(256) void gtd_attention_kernel(const double* __restrict__ hproj, const double* __restrict__ sproj,
                                                            int ks, size_t slab, const float* __restrict__ proj, const float* __restrict__ wa,
                                                            const float* __restrict__ if_pre, const double* __restrict__ h1t,
                                                            const double* __restrict__ h2t, const double* __restrict__ st,
                                                            double* __restrict__ att, double* __restrict__ beta,
                                                            double* __restrict__ ctx, double* __restrict__ chat,
                                                            double* __restrict__ xh2, double* __restrict__ x2t, int step,
                                                            int Tm, int L, int H) {
  extern __shared__ double gsm[];
  double* hp = gsm;
  double* sp = gsm + H;
  double* pre = gsm + 2 * H;
  const int b = blockIdx.x, S = Tm + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < H; j += 256) {
    double hv = hproj[(size_t)b * H + j], sv = sproj[(size_t)b * H + j];
    for (int q = 1; q < ks; ++q) { hv += hproj[(size_t)q * slab + (size_t)b * H + j]; sv += sproj[(size_t)q * slab + (size_t)b * H + j]; }
    hp[j] = hv; sp[j] = sv;
  }
  __syncthreads();
  for (int l = wave; l <= L; l += 4) {
    double p = 0.0;
    if (l < L) {
      const float* prow = proj + ((size_t)b * L + l) * H;
      for (int j = lane; j < H; j += 64) p += tanh((double)prow[j] + hp[j]) * (double)wa[j];
    } else {
      for (int j = lane; j < H; j += 64) p += tanh(sp[j] + hp[j]) * (double)wa[j];
    }
    p = wave_sum_d(p);
    if (lane == 0) pre[l] = p;
  }
  __syncthreads();
  const size_t row = (size_t)b * S + step + 1;
  if (wave == 0) {
    double mx = -1e300;
    for (int l = lane; l < L; l += 64) mx = fmax(mx, pre[l]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    double sm = 0.0;
    for (int l = lane; l < L; l += 64) sm += exp(pre[l] - mx);
    sm = wave_sum_d(sm);
    const double zt = pre[L], mx2 = fmax(mx, zt);
    double sm2 = 0.0;
    for (int l = lane; l < L; l += 64) sm2 += exp(pre[l] - mx2);
    sm2 = wave_sum_d(sm2);
    const double ez = exp(zt - mx2), bt = ez / (sm2 + ez);
    for (int l = lane; l < L; l += 64) {
      const double al = exp(pre[l] - mx) / sm;
      pre[l] = al;
      att[row * L + l] = al;
    }
    if (lane == 0) { pre[L] = bt; beta[row] = bt; }
  }
  __syncthreads();
  const double bt = pre[L];
  for (int j = tid; j < H; j += 256) {
    double c = 0.0;
    for (int l = 0; l < L; ++l) c += pre[l] * (double)fmaxf(if_pre[((size_t)b * L + l) * H + j], 0.f);
    const double ch = bt * st[row * H + j] + (1.0 - bt) * c;
    const double h1 = h1t[row * H + j];
    ctx[row * H + j] = c;
    chat[row * H + j] = ch;
    double* x = xh2 + (size_t)b * 3 * H;
    x[j] = ch;
    x[H + j] = h1;
    x[2 * H + j] = h2t[((size_t)b * S + step) * H + j];
    x2t[((size_t)b * Tm + step) * 2 * H + j] = ch;
    x2t[((size_t)b * Tm + step) * 2 * H + H + j] = h1;
  }
}

// Tail (E:1307-1319) with the attention-sum rule accumulated over every step (E:1292-1299): A operand of the tail GEMM
// (see tail_a_kernel in decoder_kernels.h).  The per-step fold with its float32 rounding after every += (E:1189, E:1293)
// and the division by stab(pre) happen here, the (L x H).(H x D) product runs on conv_igemm with the F-multiply as its
// gate, tail_finish_kernel adds the mean-pool share.
//   r_V[l][j] = fold_{i=t-1..0} float32( r_V + relu(if_pre[l][j]) * att[i+1][l] * rho[i][j] )
//   A[n][l][j] = float32( r_V[l][j] / stab(if_pre[l][j]) )
__global__ __launch_bounds__(256) void gtd_tail_a_kernel(const int* __restrict__ img_idx, const int* __restrict__ tpos,
                                                         const float* __restrict__ if_pre, const double* __restrict__ att,
                                                         const double* __restrict__ rho, float* __restrict__ A, int Tm,
                                                         int L, int H) {
  const int n = blockIdx.y, b = img_idx[n], t = tpos[n], S = Tm + 1, H8 = H >> 3;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < L * H8; idx += gridDim.x * 256) {
    const int l = idx / H8, j0 = (idx - l * H8) << 3;
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float pre = if_pre[((size_t)b * L + l) * H + j0 + q];
      const double vf = (double)fmaxf(pre, 0.f);
      float rV = 0.f;
      for (int i = t - 1; i >= 0; --i)
        rV = (float)((double)rV + vf * att[((size_t)b * S + i + 1) * L + l] * rho[((size_t)n * Tm + i) * H + j0 + q]);
      v[q] = (float)((double)rV / stab((double)pre));
    }
    float* dst = A + ((size_t)n * L + l) * H + j0;
    *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(v);
    *reinterpret_cast<f32x4*>(dst + 4) = *reinterpret_cast<const f32x4*>(v + 4);
  }
}

}  // namespace lrp
