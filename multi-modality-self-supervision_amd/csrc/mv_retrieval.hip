// Image-report retrieval (the reference's Downstream_task/Retrieval/full_dset_retrieval.py) from device-resident banks:
//   mv_pair_negatives  the training sampler of CXR_Retrieval_Dataset.__getitem__ (:108-143) on explicit 32-bit draws
//   mv_pair_assemble   pair batches (text rows, segment, 1-D mask descriptors, gathered region features) from index lists
//   mv_rank_groups     ITM logits of a whole evaluation -> P(aligned), position in the group's order, rank of the first aligned candidate
//                      and the sums behind Hit@k / MRR / recall@k / precision@k (compute_ranks :250-275, compute_recall_precision :277-314)
// Integer and copy work plus one O(C^2) count per group: one block per pair / group, candidates tiled through LDS.
//
// ORDER WITHIN A GROUP.  Candidates are ordered by descending p (the f32 value this kernel writes), exact ties by the HIGHER candidate
// index first, NaN after every number (among NaNs again the higher index first).  That is what reversing a stable ascending sort
// gives -- the reference's np.argsort(sim)[::-1]; numpy's default sort is stable for short arrays only, so beyond that the reference's
// order among exact ties is unspecified and this rule is the definition.  (numpy itself would put a NaN FIRST after the reversal; a NaN
// score is a broken candidate and is ranked last here.)
#include "mv_bank.h"

namespace {
using namespace mv_bank;              // NT: every block of this file

constexpr int NW = NT / 64;
constexpr int MAX_DRAWS = 300;        // the reference's `for itr in range(300)` (:119)
constexpr int FAMILY_1D = 4;

// ---------------------------------------------------------------------------------------------------- sampler
// draw t of sample i: two words of the counter-based hash at counters 2c and 2c + 1, c = i * 300 + t
__device__ __forceinline__ void pair_draw(unsigned k0, unsigned k1, int i, int t, unsigned& w0, unsigned& w1) {
  const unsigned c = (unsigned)i * (unsigned)MAX_DRAWS + (unsigned)t;
  w0 = mv_hash32(2u * c, k0, k1);
  w1 = mv_hash32(2u * c + 1u, k0, k1);
}

__global__ void pair_draws_kernel(unsigned k0, unsigned k1, int B, int D, uint32_t* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * D) return;
  unsigned w0, w1;
  pair_draw(k0, k1, e / D, e % D, w0, w1);
  out[2 * (size_t)e] = w0;
  out[2 * (size_t)e + 1] = w1;
}

__global__ void pair_negatives_kernel(const int32_t* __restrict__ idx, int B, int n, const int32_t* __restrict__ class_id, unsigned k0,
                                      unsigned k1, const uint32_t* __restrict__ draws, int n_draws, int32_t* __restrict__ pairs,
                                      int32_t* __restrict__ labels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int d = min(max(idx[i], 0), n - 1);            // (an index outside the dataset is clamped: nothing is read out of bounds)
  const int tries = class_id ? (draws ? min(n_draws, MAX_DRAWS) : MAX_DRAWS) : 1;
  const int cd = class_id ? class_id[d] : 0;
  int other = 0;
  unsigned w0 = 0, w1 = 0;
  for (int t = 0; t < tries; ++t) {
    if (draws) {
      w0 = draws[2 * ((size_t)i * n_draws + t)];
      w1 = draws[2 * ((size_t)i * n_draws + t) + 1];
    } else {
      pair_draw(k0, k1, i, t, w0, w1);
    }
    const int r = (int)(((unsigned long long)w0 * (unsigned long long)(n - 1)) >> 32);     // random.choice over the n - 1 other items
    other = r + (r >= d ? 1 : 0);
    if (!class_id || class_id[other] != cd) break;      // label_conditioned: a negative of another class (else: the last draw is kept)
  }
  const bool swap_img = (w1 >> 31) != 0;                // random.random() > 0.5 -> the random IMAGE with the sample's own text
  pairs[2 * i] = d;
  pairs[2 * i + 1] = d;
  pairs[2 * (B + i)] = swap_img ? other : d;
  pairs[2 * (B + i) + 1] = swap_img ? d : other;
  labels[i] = 1;
  labels[B + i] = 0;
}

// ---------------------------------------------------------------------------------------------------- pair batches
// grid (R, chunks): every block of a pair copies one chunk of its feature row; chunk 0 also writes the text side.
template <typename E>
__global__ __launch_bounds__(NT) void pair_assemble_kernel(const int64_t* __restrict__ txt_ids, const int32_t* __restrict__ txt_len,
                                                           int T_items, const E* __restrict__ img, int I_items,
                                                           const int64_t* __restrict__ img_pos, const int32_t* __restrict__ pairs, int N,
                                                           int S, int64_t* __restrict__ input_txt, int64_t* __restrict__ segment,
                                                           int32_t* __restrict__ n_ids, int32_t* __restrict__ desc,
                                                           E* __restrict__ feats, int64_t* __restrict__ pos_out, ChunkPlan plan) {
  const int r = blockIdx.x, T = S + 1;
  const int im = clamp_item(pairs[2 * r], I_items);
  const int tx = clamp_item(pairs[2 * r + 1], T_items);
  if (blockIdx.y == 0) {
    const int64_t* src = txt_ids + (size_t)tx * T;
    for (int t = threadIdx.x; t < T; t += NT) {
      input_txt[(size_t)r * T + t] = src[t];
      segment[(size_t)r * T + t] = 1;                             // full_dset_retrieval.py:203: ones over all S + 1 positions
    }
    copy_pos_row(img_pos, im, pos_out, r, N);
    if (threadIdx.x == 0) {
      const int len = min(max(txt_len[tx], 0), T);
      n_ids[r] = len;
      write_desc(desc, r, FAMILY_1D, N, len);
    }
  }
  copy_chunk(img + (size_t)im * plan.row, feats + (size_t)r * plan.row, plan.row, blockIdx.y * plan.chunk, plan.chunk, plan.vec);
}

// ---------------------------------------------------------------------------------------------------- ranking
struct RankKs {
  int nk;
  int k[8];
};

__device__ __forceinline__ int block_sum_i(int v, int* s_red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if (lane == 0) s_red[wid] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += s_red[w];
  return t;
}
__device__ __forceinline__ int block_min_i(int v, int* s_red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  __syncthreads();
  if (lane == 0) s_red[wid] = v;
  __syncthreads();
  int t = s_red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = min(t, s_red[w]);
  return t;
}

// sort key: p lies in [0, 1]; a NaN goes below every number
__device__ __forceinline__ float rank_key(float p) { return p != p ? -1.0f : p; }
// 32.32 fixed point of a ratio in [0, 1], rounded to nearest even: integer sums do not depend on the order of the groups
__device__ __forceinline__ unsigned long long rank_fx(double x) { return (unsigned long long)rint(ldexp(x, 32)); }

// one block per group
__global__ __launch_bounds__(NT) void rank_groups_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int C, RankKs ks,
                                                         float* __restrict__ p_out, int32_t* __restrict__ pos_out,
                                                         int32_t* __restrict__ rank_out, unsigned long long* __restrict__ counters) {
  __shared__ float s_key[NT];
  __shared__ int s_red[NW];
  const size_t base = (size_t)blockIdx.x * C;
  const int tid = threadIdx.x;
  // 1. P(aligned) = softmax(logits)[1] in f32, written out: everything below ranks the written value
  for (int i = tid; i < C; i += NT) {
    const float l0 = logits[2 * (base + i)], l1 = logits[2 * (base + i) + 1];
    const float m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m);
    float p = e1 / (e0 + e1);
    if (l0 != l0 || l1 != l1) p = __builtin_nanf("");
    p_out[base + i] = p;
  }
  __syncthreads();                   // (the block's own global writes are visible to it after the barrier)
  // 2. pos = candidates ahead of this one; the group's keys pass through LDS a tile at a time
  int best = C, n_al = 0;
  int topk[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) topk[q] = 0;
  for (int i0 = 0; i0 < C; i0 += NT) {
    const int i = i0 + tid;
    const bool mine = i < C;
    const float ki = mine ? rank_key(p_out[base + i]) : 0.f;
    int cnt = 0;
    for (int j0 = 0; j0 < C; j0 += NT) {
      __syncthreads();
      if (j0 + tid < C) s_key[tid] = rank_key(p_out[base + j0 + tid]);
      __syncthreads();
      const int nj = min(NT, C - j0);
      for (int jj = 0; jj < nj; ++jj) {
        const float kj = s_key[jj];
        cnt += (kj > ki || (kj == ki && j0 + jj > i)) ? 1 : 0;
      }
    }
    if (mine) {
      pos_out[base + i] = cnt;
      if (labels[base + i] == 1) {
        ++n_al;
        best = min(best, cnt);
#pragma unroll
        for (int q = 0; q < 8; ++q) topk[q] += (q < ks.nk && cnt < ks.k[q]) ? 1 : 0;
      }
    }
  }
  // 3. the group's rank and its terms of the sums
  const int rank = block_min_i(best, s_red);
  const int total = block_sum_i(n_al, s_red);
  int tk[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) tk[q] = q < ks.nk ? block_sum_i(topk[q], s_red) : 0;
  if (tid == 0) {
    rank_out[blockIdx.x] = rank;
    atomicAdd(&counters[0], 1ull);
    if (total == 0) atomicAdd(&counters[1], 1ull);
    atomicAdd(&counters[2], rank_fx(1.0 / (double)(rank + 1)));
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (q >= ks.nk) continue;
      if (rank < ks.k[q]) atomicAdd(&counters[4 + q], 1ull);
      if (total > 0) atomicAdd(&counters[12 + q], rank_fx((double)tk[q] / (double)total));
      atomicAdd(&counters[20 + q], (unsigned long long)tk[q]);
    }
  }
}

}  // namespace

extern "C" int mv_pair_draws(unsigned long long key, unsigned long long step, int B, int D, uint32_t* draws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!draws || B <= 0 || D <= 0) return MV_E_ARG;
  if (D > MAX_DRAWS || (long long)B * MAX_DRAWS > 0x3fffffffLL) return MV_E_SHAPE;
  unsigned k0, k1;
  mv_derive_keys(key, step, k0, k1);
  const int n = B * D;
  pair_draws_kernel<<<(n + 255) / 256, 256, 0, stream>>>(k0, k1, B, D, draws);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_pair_negatives(const int32_t* idx, int B, int n, const int32_t* class_id, unsigned long long key, unsigned long long step,
                                 const uint32_t* draws, int n_draws, int32_t* pairs, int32_t* labels, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!idx || !pairs || !labels || B <= 0 || n < 2) return MV_E_ARG;
  if (draws && n_draws <= 0) return MV_E_ARG;
  if ((long long)B * MAX_DRAWS > 0x3fffffffLL) return MV_E_SHAPE;          // 32-bit hash counters, int32 pair offsets
  unsigned k0, k1;
  mv_derive_keys(key, step, k0, k1);
  pair_negatives_kernel<<<(B + 255) / 256, 256, 0, stream>>>(idx, B, n, class_id, k0, k1, draws, n_draws, pairs, labels);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_pair_assemble(const int64_t* txt_ids, const int32_t* txt_len, int T_items, const void* img_feats, int dtype, int I_items,
                                const int64_t* img_pos, const int32_t* pairs, int R, int N, int S, int F, int64_t* input_txt,
                                int64_t* segment, int32_t* n_ids, int32_t* desc, void* feats, int64_t* pos_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!txt_ids || !txt_len || !img_feats || !pairs || !input_txt || !segment || !n_ids || !desc || !feats) return MV_E_ARG;
  if (T_items <= 0 || I_items <= 0 || R <= 0 || N <= 0 || S <= 0 || F <= 0) return MV_E_ARG;
  if ((img_pos != nullptr) != (pos_out != nullptr)) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if ((long long)N * F > 0x7fffffffLL || R > 0x3fffffff) return MV_E_SHAPE;
  typedef mv_types<float, bf16_t, f16_t> Accept;      // f16 runs the bf16 instantiation: 2-byte elements move as bits (mv_bits_t)
  return mv_with_type(dtype, Accept{}, [&](auto t) -> int {
    typedef mv_bits_t<MV_T(t)> E;
    const ChunkPlan p = chunk_plan((unsigned)((long long)N * F), sizeof(E), img_feats, feats);
    hipLaunchKernelGGL(pair_assemble_kernel<E>, dim3((unsigned)R, p.chunks), dim3(NT), 0, stream, txt_ids, txt_len, T_items,
                       (const E*)img_feats, I_items, img_pos, pairs, N, S, input_txt, segment, n_ids, desc, (E*)feats, pos_out, p);
    return (int)hipGetLastError();
  });
}

extern "C" int mv_rank_groups(const float* logits, const int32_t* labels, int G, int C, const int32_t* ks, int nk, float* p, int32_t* pos,
                              int32_t* rank, unsigned long long* counters, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !p || !pos || !rank || !counters || G <= 0 || C < 1 || nk < 0 || (nk > 0 && !ks)) return MV_E_ARG;
  if (nk > 8) return MV_E_ARG;
  RankKs kk;
  kk.nk = nk;
  for (int q = 0; q < 8; ++q) {
    kk.k[q] = q < nk ? ks[q] : 0;                        // ks is a HOST array
    if (q < nk && ks[q] <= 0) return MV_E_ARG;
  }
  if ((long long)G * C > 0x3fffffffLL) return MV_E_SHAPE;
  rank_groups_kernel<<<G, NT, 0, stream>>>(logits, labels, C, kk, p, pos, rank, counters);
  MV_CHECK_LAUNCH();
  return MV_OK;
}
