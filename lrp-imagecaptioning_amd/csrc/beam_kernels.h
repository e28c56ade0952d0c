// beam_kernels.h — the beam bookkeeping of the caption search (E:51-120, models/explainers.py; batched form
// inference.py:178-253) on the device, exactly as beam.search (beam.py) restates it: one search step for all images in one
// launch, so that the decoder loop needs no host between its steps (Decoder::beam_search, lrp_op_beam_select / _finish).
//
// Per image the state holds, in two buffers (a step reads buffer s & 1 and writes the other: parents permute, and the
// complete set is re-ranked):
//   * the live set: k sentences (int32 tokenizer ids, max_len slots each) and their float64 log-probabilities, in
//     descending order — after the re-parenting of a step, live hypothesis j is computed in row j of the image;
//   * the complete set: <= k sentences, their lengths and float64 log-probabilities, in descending order; its count.
// A step has k candidates at s = 0 (only row 0 is live, E:60-64) and k * k afterwards: total = live_lp + logp in float64,
// sentence = parent's sentence + (id + 1).  It keeps the k LARGEST under the reference's total order (log_prob, sentence)
// — `Caption` tuple comparison, inference.py:297-315: on an exact tie of the log-probabilities the lexicographically larger
// word sequence, a proper prefix being the smaller — and ALSO records every candidate whose new word is EOS as a complete
// caption (the sentence before the EOS, the candidate's total), under the same order, truncated to k.  A candidate that
// just produced EOS keeps competing for a live slot (E:88-93).
//
// Selection is a rank by counting over keys in LDS: rank(c) = number of candidates above c; rank < k is the output slot.
// No atomics and no float32: the result is the same bits run to run, and the same as the host's sort.  A tie of the totals
// is decided by an integer key (rank of the parent's sentence among the live sentences, new word): candidates of one
// step have equal lengths, so comparing them is comparing the parents and then the words.  Complete captions of
// different steps have different lengths; they meet the new ones in `above_complete`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace lrp {

constexpr int BEAM_K_MAX = 32;                        // = TOPK_MAX (score_kernels.h): what the ranking kernel can feed
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_CAND_MAX = BEAM_K_MAX * BEAM_K_MAX;

// One buffer of one image: [live_lp k f64 | comp_lp k f64 | live_sent k*T i32 | comp_sent k*T i32 | comp_len k i32 | n_comp, pad].
struct BeamView {
  double* live_lp;
  double* comp_lp;
  int* live_sent;
  int* comp_sent;
  int* comp_len;
  int* n_comp;
};
__host__ __device__ inline size_t beam_buffer_bytes(int k, int T) {
  const size_t b = (size_t)2 * k * sizeof(double) + ((size_t)2 * k * T + k + 2) * sizeof(int);
  return (b + 7) / 8 * 8;
}
__host__ __device__ inline size_t beam_state_bytes(int n_images, int k, int T) {
  return (size_t)n_images * 2 * beam_buffer_bytes(k, T);
}
__device__ inline BeamView beam_view(void* state, int image, int buf, int k, int T) {
  char* p = static_cast<char*>(state) + ((size_t)image * 2 + buf) * beam_buffer_bytes(k, T);
  BeamView v;
  v.live_lp = reinterpret_cast<double*>(p);
  v.comp_lp = v.live_lp + k;
  v.live_sent = reinterpret_cast<int*>(v.comp_lp + k);
  v.comp_sent = v.live_sent + (size_t)k * T;
  v.comp_len = v.comp_sent + (size_t)k * T;
  v.n_comp = v.comp_len + k;
  return v;
}

// is the new complete caption (total tn, sentence = the first s words of `sent`) above the recorded one (te, ce, le words)?
// The recorded ones come from earlier steps, le < s: when the first le words agree the recorded one is a proper prefix.
__device__ inline bool above_complete(double tn, const int* __restrict__ sent, double te, const int* __restrict__ ce, int le) {
  if (tn != te) return tn > te;
  for (int x = 0; x < le; ++x)
    if (sent[x] != ce[x]) return sent[x] > ce[x];
  return true;
}

// grid = n_images, 256 threads.  ids / logp (n_images * k, k) as log_softmax_topk_kernel writes them; parent_out / word_out
// (n_images * k): row i * k + q of the next step continues row parent_out (a row of the same image) with tokenizer id word_out.
__global__ __launch_bounds__(BEAM_THREADS) void beam_select_kernel(void* __restrict__ state, const int* __restrict__ ids,
                                                                  const double* __restrict__ logp, int k, int T, int s, int eos,
                                                                  int* __restrict__ parent_out, int* __restrict__ word_out) {
  __shared__ double tot[BEAM_CAND_MAX];
  __shared__ long long key[BEAM_CAND_MAX];              // (rank of the parent's sentence) << 32 | word: the order inside a tie
  __shared__ unsigned char sent_gt[BEAM_CAND_MAX];      // sent_gt[a * k + b]: live sentence a > live sentence b
  __shared__ int prank[BEAM_K_MAX];
  const int tid = threadIdx.x, img = blockIdx.x;
  const BeamView cur = beam_view(state, img, s & 1, k, T), nxt = beam_view(state, img, (s + 1) & 1, k, T);
  const int n_live = s == 0 ? 1 : k;                    // k <= V: step 0 always fills the beam
  const int n_cand = n_live * k;
  // (counts and lengths are clamped: a state that did not start at step 0 gives wrong captions, never a wild read)
  const int n_comp = s == 0 ? 0 : min(max(*cur.n_comp, 0), k);

  // order of the live sentences (s words each); distinct by construction, the order is strict
  for (int t = tid; t < n_live * n_live; t += BEAM_THREADS) {
    const int a = t / n_live, b = t % n_live;
    const int *sa = cur.live_sent + (size_t)a * T, *sb = cur.live_sent + (size_t)b * T;
    bool gt = false;
    for (int x = 0; x < s; ++x)
      if (sa[x] != sb[x]) { gt = sa[x] > sb[x]; break; }
    sent_gt[t] = gt;
  }
  __syncthreads();
  if (tid < n_live) {
    int r = 0;
    for (int b = 0; b < n_live; ++b) r += sent_gt[tid * n_live + b];
    prank[tid] = r;
  }
  __syncthreads();
  for (int c = tid; c < n_cand; c += BEAM_THREADS) {
    const int p = c / k;
    const double lp = s == 0 ? 0.0 : cur.live_lp[p];
    tot[c] = lp + logp[(size_t)img * k * k + c];        // IEEE float64 add, as `lp + float(l)` on the host
    key[c] = ((long long)prank[p] << 32) | ((unsigned int)ids[(size_t)img * k * k + c] + 1u);
  }
  __syncthreads();

  // ranks by counting.  above(j, c): (tot, key) larger, the earlier candidate on a full tie (the host's stable sort)
  int n_new = 0;                                        // candidates that end in EOS (uniform: counted at a barrier)
  for (int base = 0; base < n_cand; base += BEAM_THREADS) {
    const int c = base + tid;
    const bool valid = c < n_cand;
    const double tc = valid ? tot[c] : 0.0;
    const long long kc = valid ? key[c] : 0;
    const bool is_eos = valid && (int)(kc & 0xffffffffLL) == eos;
    int rank = 0, crank = 0;
    if (valid) {
      for (int j = 0; j < n_cand; ++j) {
        const double tj = tot[j];
        const long long kj = key[j];
        const bool ab = tj > tc || (tj == tc && (kj > kc || (kj == kc && j < c)));
        rank += ab;
        crank += ab && (int)(kj & 0xffffffffLL) == eos;
      }
    }
    if (valid && rank < k) {                            // live slot `rank` of the next step
      const int p = c / k, w = (int)(kc & 0xffffffffLL);
      const int* src = cur.live_sent + (size_t)p * T;
      int* dst = nxt.live_sent + (size_t)rank * T;
      for (int x = 0; x < s; ++x) dst[x] = src[x];
      dst[s] = w;
      nxt.live_lp[rank] = tc;
      parent_out[img * k + rank] = img * k + p;
      word_out[img * k + rank] = w;
    }
    if (is_eos && crank < k) {                          // a new complete caption: the parent's sentence, the candidate's total
      const int* src = cur.live_sent + (size_t)(c / k) * T;
      for (int e = 0; e < n_comp; ++e) crank += !above_complete(tc, src, cur.comp_lp[e], cur.comp_sent + (size_t)e * T, min(max(cur.comp_len[e], 0), s));
      if (crank < k) {
        int* dst = nxt.comp_sent + (size_t)crank * T;
        for (int x = 0; x < s; ++x) dst[x] = src[x];
        nxt.comp_len[crank] = s;
        nxt.comp_lp[crank] = tc;
      }
    }
    n_new += __syncthreads_count(is_eos);
  }
  // the recorded complete captions keep their order and move down by the number of new ones above them
  if (tid < n_comp) {
    const double te = cur.comp_lp[tid];
    const int* ce = cur.comp_sent + (size_t)tid * T;
    const int le = min(max(cur.comp_len[tid], 0), s);
    int rank = tid;
    for (int j = 0; j < n_cand && rank < k; ++j)
      if ((int)(key[j] & 0xffffffffLL) == eos) rank += above_complete(tot[j], cur.live_sent + (size_t)(j / k) * T, te, ce, le);
    if (rank < k) {
      int* dst = nxt.comp_sent + (size_t)rank * T;
      for (int x = 0; x < le; ++x) dst[x] = ce[x];
      nxt.comp_len[rank] = le;
      nxt.comp_lp[rank] = te;
    }
  }
  if (tid == 0) *nxt.n_comp = n_comp + n_new < k ? n_comp + n_new : k;
}

// What beam.search returns after `steps` steps: per image k captions — the complete ones by descending order, then live ones —
// each with a trailing EOS.  captions (n_images, k, T + 1) zero-padded, lengths (n_images, k) EOS included, logp (n_images, k),
// n_complete (n_images).  grid = n_images, 64 threads.
__global__ __launch_bounds__(64) void beam_finish_kernel(const void* __restrict__ state, int k, int T, int steps, int eos,
                                                         int* __restrict__ captions, int* __restrict__ lengths,
                                                         double* __restrict__ logp, int* __restrict__ n_complete) {
  const int img = blockIdx.x;
  const BeamView v = beam_view(const_cast<void*>(state), img, steps & 1, k, T);
  const int n_comp = min(max(*v.n_comp, 0), k);
  for (int t = threadIdx.x; t < k * (T + 1); t += 64) {
    const int q = t / (T + 1), x = t % (T + 1);
    const bool comp = q < n_comp;
    const int len = comp ? min(max(v.comp_len[q], 0), T) : steps;
    const int* sent = comp ? v.comp_sent + (size_t)q * T : v.live_sent + (size_t)(q - n_comp) * T;
    captions[((size_t)img * k + q) * (T + 1) + x] = x < len ? sent[x] : (x == len ? eos : 0);
    if (x == 0) {
      lengths[img * k + q] = len + 1;
      logp[img * k + q] = comp ? v.comp_lp[q] : v.live_lp[q - n_comp];
    }
  }
  if (threadIdx.x == 0) n_complete[img] = n_comp;
}

}  // namespace lrp
