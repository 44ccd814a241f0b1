// Corpus BLEU-1..4 of generated reports, counted on the device (the reference's evaluation, Downstream_task/report_generation_and_vqa/
// sc/generation_decode.py:480-498 with detokenize :97-104 and sc/bleu.py:16-64, which hands the word lists to nltk's corpus_bleu):
//   mv_bleu_words    token ids -> the 64-bit key of every word of ' '.join(detokenize(tokens before [SEP] / [PAD])).split(' ')
//   mv_bleu_counts   hypothesis and reference word keys -> the ten integers corpus_bleu's four scores follow from
// A word's key is the polynomial hash of its UTF-8 bytes modulo 2^64 (report_eval.py), so that the key of a word assembled from word
// pieces follows from the pieces' keys: key(a + b) = key(a) P^len(b) + key(b).  Equal keys are taken for equal words.  Integer work:
// mv_bleu_words accumulates nothing, mv_bleu_counts adds each block's counts with 64-bit integer atomics, so its sums do not depend on
// the order in which blocks finish.
#include "mv_bank.h"

namespace {
using namespace mv_bank;
typedef unsigned long long u64;

constexpr int MAX_T = 1024;           // tokens / words per row
constexpr int MAX_V = 1 << 20;        // vocabulary entries
constexpr int MAX_N = 1 << 20;        // rows of one launch
constexpr int NORD = 4;               // BLEU-1 .. BLEU-4
constexpr int NCOUNT = 10;            // num_1..4, den_1..4, hyp_len, ref_len

// One block per row.  Pass 1 finds the row's end and writes a (pow, key) pair per kept token into LDS: (0, tok_key) for a token that
// starts a word, (tail_pow, tail_key) for one that extends it.  Pass 2 numbers the word starts (ballot + popcount per wave, the waves'
// totals through LDS) and the lane of a start walks its continuations: words of reports are one to three pieces long, and the longest
// walk, T - 1 steps of a multiply-add out of LDS, is bounded by T <= 1024.
__global__ __launch_bounds__(NT) void bleu_words_kernel(const int64_t* __restrict__ ids, int ld, int T, const u64* __restrict__ tok_key,
                                                        const u64* __restrict__ tail_key, const u64* __restrict__ tail_pow, int V,
                                                        int64_t eos_id, int64_t pad_id, u64 empty_key, u64* __restrict__ word_key,
                                                        int32_t* __restrict__ n_words) {
  __shared__ u64 s_key[MAX_T];
  __shared__ u64 s_pow[MAX_T];
  __shared__ int s_end;
  __shared__ int s_wave[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t* row = ids + (size_t)blockIdx.x * ld;
  u64* out = word_key + (size_t)blockIdx.x * T;
  if (tid == 0) s_end = T;
  __syncthreads();
  for (int t = tid; t < T; t += NT) {
    const int64_t id = row[t];
    if (id == eos_id || id == pad_id || id < 0 || id >= V) {         // (an id outside the tables ends the row as [PAD] does)
      atomicMin(&s_end, t);
    } else {
      const u64 pw = tail_pow[id];
      const bool cont = pw != 0 && t > 0;                            // a leading ##x keeps its ## (detokenize: len(r_list) > 0)
      s_pow[t] = cont ? pw : 0;
      s_key[t] = cont ? tail_key[id] : tok_key[id];
    }
  }
  __syncthreads();
  const int end = s_end;                                             // kept tokens: [0, end), all of them written above
  int n = 0;
  for (int t0 = 0; t0 < end; t0 += NT) {                             // (uniform over the block)
    const int t = t0 + tid;
    const bool start = t < end && s_pow[t] == 0;
    const u64 b = __ballot(start);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int w = n + __popcll(b & ((1ull << lane) - 1ull));
    for (int k = 0; k < NT / 64; ++k) {
      if (k < wave) w += s_wave[k];
      n += s_wave[k];
    }
    if (start) {
      u64 key = s_key[t];
      for (int u = t + 1; u < end && s_pow[u] != 0; ++u) key = key * s_pow[u] + s_key[u];
      out[w] = key;                                                  // w < number of starts <= end <= T
    }
    __syncthreads();                                                 // (the next pass rewrites s_wave)
  }
  if (end == 0) {                                                    // ''.split(' ') == ['']: one empty word
    n = 1;
    if (tid == 0) out[0] = empty_key;
  }
  for (int t = n + tid; t < T; t += NT) out[t] = 0;
  if (tid == 0) n_words[blockIdx.x] = n;
}

// The words of `s` (L of them, three readable words behind) against the o-grams that start at one hypothesis position: w[0..ap) are
// its words.  cnt[o] counts the positions q whose first o + 1 words equal w's; bit o of `before` is set when such a q lies below p.
// q is uniform over the wave: every LDS read is a broadcast.
__device__ __forceinline__ void match_row(const u64* s, int L, const u64 (&w)[NORD], int ap, int p, unsigned (&cnt)[NORD], unsigned& before) {
  u64 a = s[0], b = s[1], c = s[2];
  for (int q = 0; q < L; ++q) {
    const u64 d = s[q + 3];
    const int lim = min(ap, L - q);                                  // orders that fit at both positions
    const unsigned m1 = a == w[0];
    const unsigned m2 = m1 & (b == w[1]) & (lim >= 2);
    const unsigned m3 = m2 & (c == w[2]) & (lim >= 3);
    const unsigned m4 = m3 & (d == w[3]) & (lim >= 4);
    cnt[0] += m1;
    cnt[1] += m2;
    cnt[2] += m3;
    cnt[3] += m4;
    if (q < p) before |= m1 | (m2 << 1) | (m3 << 2) | (m4 << 3);
    a = b;
    b = c;
    c = d;
  }
}

// One block per sample, both word rows in LDS.  A lane takes the hypothesis positions p = tid, tid + NT, ...; for each it decides per
// order whether p is the first occurrence of its o-gram and counts the o-gram on both sides, in one pass over each row for all four
// orders (the n words are compared one by one).
__global__ __launch_bounds__(NT) void bleu_counts_kernel(const u64* __restrict__ hyp_key, int Th, const int32_t* __restrict__ hyp_n,
                                                         const u64* __restrict__ ref_key, int Tr, const int32_t* __restrict__ ref_n,
                                                         int n_items, const int32_t* __restrict__ idx, u64* __restrict__ counters) {
  __shared__ u64 s_h[MAX_T + NORD - 1];
  __shared__ u64 s_r[MAX_T + NORD - 1];
  __shared__ u64 s_red[NT / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int d = clamp_item(idx[i], n_items);
  const int Lh = min(max(hyp_n[i], 0), Th), Lr = min(max(ref_n[d], 0), Tr);
  for (int t = tid; t < Lh + NORD - 1; t += NT) s_h[t] = t < Lh ? hyp_key[(size_t)i * Th + t] : 0;     // (the tail is read, never matched)
  for (int t = tid; t < Lr + NORD - 1; t += NT) s_r[t] = t < Lr ? ref_key[(size_t)d * Tr + t] : 0;
  __syncthreads();

  unsigned num[NORD] = {0, 0, 0, 0};
  for (int p = tid; p < Lh; p += NT) {
    const int ap = min(NORD, Lh - p);                                // orders of which an o-gram starts at p
    const u64 w[NORD] = {s_h[p], s_h[p + 1], s_h[p + 2], s_h[p + 3]};
    unsigned ch[NORD] = {0, 0, 0, 0}, cr[NORD] = {0, 0, 0, 0}, before = 0, unused = 0;
    match_row(s_h, Lh, w, ap, p, ch, before);
    match_row(s_r, Lr, w, ap, 0, cr, unused);
#pragma unroll
    for (int o = 0; o < NORD; ++o)
      if (o < ap && !((before >> o) & 1u)) num[o] += min(ch[o], cr[o]);                                // clipped by the reference's count
  }
#pragma unroll
  for (int o = 0; o < NORD; ++o) block_add(num[o], counters + o, s_red);
  if (tid == 0) {
    for (int o = 0; o < NORD; ++o) atomicAdd(counters + NORD + o, (u64)max(1, Lh - o));                // nltk's modified_precision
    if (Lh) atomicAdd(counters + 2 * NORD, (u64)Lh);
    if (Lr) atomicAdd(counters + 2 * NORD + 1, (u64)Lr);
  }
}

}  // namespace

extern "C" int mv_bleu_words(const int64_t* ids, int ld, int n, int T, const int64_t* tok_key, const int64_t* tail_key,
                             const int64_t* tail_pow, int V, int64_t eos_id, int64_t pad_id, int64_t empty_key, int64_t* word_key,
                             int32_t* n_words, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ids || !tok_key || !tail_key || !tail_pow || !word_key || !n_words) return MV_E_ARG;
  if (n <= 0 || T <= 0 || V <= 0 || ld < T) return MV_E_ARG;
  if (T > MAX_T || V > MAX_V || n > MAX_N) return MV_E_SHAPE;
  bleu_words_kernel<<<dim3((unsigned)n), NT, 0, stream>>>(ids, ld, T, (const u64*)tok_key, (const u64*)tail_key, (const u64*)tail_pow, V,
                                                          eos_id, pad_id, (u64)empty_key, (u64*)word_key, n_words);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_bleu_counts(const int64_t* hyp_key, int Th, const int32_t* hyp_n, int n, const int64_t* ref_key, int Tr,
                              const int32_t* ref_n, int n_items, const int32_t* idx, unsigned long long* counters, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!hyp_key || !hyp_n || !ref_key || !ref_n || !idx || !counters) return MV_E_ARG;
  if (n <= 0 || n_items <= 0 || Th <= 0 || Tr <= 0) return MV_E_ARG;
  if (Th > MAX_T || Tr > MAX_T || n > MAX_N) return MV_E_SHAPE;
  static_assert(NCOUNT == 2 * NORD + 2, "num and den per order, then the two lengths");
  bleu_counts_kernel<<<dim3((unsigned)n), NT, 0, stream>>>((const u64*)hyp_key, Th, hyp_n, (const u64*)ref_key, Tr, ref_n, n_items, idx,
                                                           counters);
  MV_CHECK_LAUNCH();
  return MV_OK;
}
