// Report fine-tuning from a device-resident bank (the reference's Preprocess4Seq2seq, Downstream_task/report_generation_and_vqa/sc/
// data_loader.py:330-419, and the row plan of report_finetune.build_plan):
//   mv_report_draws     the masking draw's random words: T shuffle keys and one coin per sample
//   mv_report_assemble  one launch per batch: the shuffle as a rank count, the [MASK] rows, the three prediction lists, segment, mask
//                       descriptors and the gathered region features
//   mv_report_plan      the lists -> the distinct consumed rows and the CSR entries over them, on the device
// Integer and copy work: every output is an integer, a copy or a 1.0, nothing is accumulated with atomics, so the same input gives the
// same bits on every run.
//
// THE DRAW.  random.shuffle of the candidates (data_loader.py:353-360) becomes "order the candidates by their 32-bit words": the rank of
// text index t is the number of candidates t' with (word[t'], t') < (word[t], t), so equal words go to the lower index and the order is
// a permutation for any words.  For independent uniform words that is a uniform shuffle up to the ties' 2^-32.
#include "mv_bank.h"

namespace {
using namespace mv_bank;

constexpr int MAX_T = 1024;           // text ids per row (LDS: T + 1 words)
constexpr int MAX_PRED = 64;          // prediction slots per sample
constexpr int PLAN_MAX_B = 2048;
constexpr int FAMILY_S2S = 1;
constexpr int64_t TOK_MASK = 103;

__global__ void report_draws_kernel(unsigned k0, unsigned k1, int n, uint32_t* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = mv_hash32((unsigned)e, k0, k1);
}

// ---------------------------------------------------------------------------------------------------- batch assembly
// grid (B, chunks): every block of a sample copies one chunk of its feature row; chunk 0 also draws the masks and writes the text side.
template <typename E>
__global__ __launch_bounds__(NT) void report_assemble_kernel(
    const int64_t* __restrict__ txt_ids, const int32_t* __restrict__ txt_len, const int32_t* __restrict__ n_pred, int n_items,
    const E* __restrict__ img, const int64_t* __restrict__ img_pos, const int32_t* __restrict__ idx, const int32_t* __restrict__ family,
    int N, int T, int max_pred, unsigned k0, unsigned k1, const uint32_t* __restrict__ draws, int64_t* __restrict__ input_txt,
    int64_t* __restrict__ segment, int32_t* __restrict__ desc, E* __restrict__ feats, int64_t* __restrict__ pos_out,
    int64_t* __restrict__ masked_pos, int64_t* __restrict__ masked_lab, float* __restrict__ masked_w, ChunkPlan plan) {
  __shared__ uint32_t s_word[MAX_T + 1];
  __shared__ int s_sel[MAX_PRED];                 // text index per slot
  __shared__ unsigned char s_listed[MAX_T];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int d = clamp_item(idx[i], n_items);
  if (blockIdx.y == 0) {
    const int len = min(max(txt_len[d], 1), T);
    const int p = max(min(min(n_pred[d], max_pred), len), 0);
    const int64_t* src = txt_ids + (size_t)d * T;
    for (int t = tid; t <= T; t += NT) {
      const size_t c = (size_t)i * (T + 1) + t;
      s_word[t] = draws ? draws[c] : mv_hash32((unsigned)c, k0, k1);
      if (t < T) s_listed[t] = 0;
    }
    __syncthreads();
    const bool coin = (s_word[T] >> 31) != 0;
    for (int t = tid; t < len; t += NT) {
      const uint32_t w = s_word[t];
      int rank = 0;
      for (int u = 0; u < len; ++u) {
        const uint32_t wu = s_word[u];
        rank += (wu < w || (wu == w && u < t)) ? 1 : 0;
      }
      if (rank < p) s_sel[rank] = t;                                // the ranks are a permutation: one writer per slot
    }
    __syncthreads();
    if (coin && p > 0 && tid == 0) s_sel[p - 1] = len - 1;          // the last [SEP] takes the final slot (it may be listed twice)
    __syncthreads();
    if (tid < max_pred) {
      const bool on = tid < p;
      const int t = on ? s_sel[tid] : 0;
      if (on) s_listed[t] = 1;                                      // (two slots with one index store the same byte)
      masked_pos[(size_t)i * max_pred + tid] = on ? (int64_t)(N + 2 + t) : 0;
      masked_lab[(size_t)i * max_pred + tid] = on ? src[t] : 0;
      masked_w[(size_t)i * max_pred + tid] = on ? 1.0f : 0.0f;
    }
    __syncthreads();
    for (int t = tid; t < T; t += NT) {
      input_txt[(size_t)i * T + t] = s_listed[t] ? TOK_MASK : src[t];
      segment[(size_t)i * T + t] = t < len ? 1 : 0;
    }
    copy_pos_row(img_pos, d, pos_out, i, N);
    if (tid == 0) write_desc(desc, i, family ? family[i] : FAMILY_S2S, N, len);
  }
  copy_chunk(img + (size_t)d * plan.row, feats + (size_t)i * plan.row, plan.row, blockIdx.y * plan.chunk, plan.chunk, plan.vec);
}

// ---------------------------------------------------------------------------------------------------- row plan
// One wave per sample, slot j on lane j.  A slot is dropped (weight 0), bad (counted, left out) or an entry.  Inside a sample the
// entries are ordered by (position, slot); samples follow each other, so the flat rows b * L + position ascend over the whole batch.
struct PlanSlot {
  bool entry, bad, first;      // first: no earlier slot of the sample lists this position
  int pos, label, rank, row;   // rank: entries of the sample ahead of this one; row: distinct positions of the sample below this one
  float w;
};

__device__ __forceinline__ PlanSlot plan_slot(const int64_t* __restrict__ pos, const int64_t* __restrict__ labels,
                                              const float* __restrict__ weights, const int32_t* __restrict__ valid_len, int b, int P, int L,
                                              int V, int* s_pos, int* s_first) {
  const int j = threadIdx.x;
  PlanSlot s = {false, false, false, 0, 0, 0, 0, 0.f};
  if (j < P) {
    const int64_t p = pos[(size_t)b * P + j], t = labels[(size_t)b * P + j];
    s.w = weights[(size_t)b * P + j];
    const bool w_ok = s.w >= 0.f && s.w <= 3.402823466e+38f;        // finite and not negative (a NaN fails both)
    if (!w_ok) {
      s.bad = true;
    } else if (s.w != 0.f) {
      const int64_t hi = valid_len ? min((int64_t)L, (int64_t)valid_len[b]) : (int64_t)L;
      s.bad = p <= 0 || p >= hi || t < 0 || t >= V;
      s.entry = !s.bad;
    }
    s.pos = s.entry ? (int)p : 0;
    s.label = s.entry ? (int)t : 0;
  }
  s_pos[j] = s.entry ? s.pos : -1;
  __syncthreads();
  if (s.entry) {
    s.first = true;
    for (int u = 0; u < P; ++u) {
      const int pu = s_pos[u];
      if (pu < 0) continue;
      s.rank += (pu < s.pos || (pu == s.pos && u < j)) ? 1 : 0;
      if (pu == s.pos && u < j) s.first = false;
    }
  }
  s_first[j] = s.first ? 1 : 0;
  __syncthreads();
  if (s.entry)
    for (int u = 0; u < P; ++u) s.row += (s_first[u] && s_pos[u] < s.pos) ? 1 : 0;
  return s;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// work int32 [B, 3] = {distinct positions, entries, bad slots} per sample
__global__ __launch_bounds__(64) void report_plan_count_kernel(const int64_t* __restrict__ pos, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ weights, const int32_t* __restrict__ valid_len,
                                                               int P, int L, int V, int32_t* __restrict__ work) {
  __shared__ int s_pos[64], s_first[64];
  const int b = blockIdx.x;
  const PlanSlot s = plan_slot(pos, labels, weights, valid_len, b, P, L, V, s_pos, s_first);
  const int u = wave_sum_i(s.first ? 1 : 0), n = wave_sum_i(s.entry ? 1 : 0), bad = wave_sum_i(s.bad ? 1 : 0);
  if (threadIdx.x == 0) {
    work[3 * b + 0] = u;
    work[3 * b + 1] = n;
    work[3 * b + 2] = bad;
  }
}

__global__ __launch_bounds__(64) void report_plan_write_kernel(const int64_t* __restrict__ pos, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ weights, const int32_t* __restrict__ valid_len,
                                                               int B, int P, int L, int V, const int32_t* __restrict__ work,
                                                               int32_t* __restrict__ rows, int32_t* __restrict__ row_ptr,
                                                               int32_t* __restrict__ out_labels, float* __restrict__ out_weights,
                                                               int32_t* __restrict__ out_sample, int32_t* __restrict__ counts) {
  __shared__ int s_pos[64], s_first[64];
  const int b = blockIdx.x, j = threadIdx.x;
  // this sample's offsets: integer sums over the samples before it (the last block sums all B for the totals)
  int u0 = 0, n0 = 0, bad = 0;
  const bool last = b == B - 1;
  for (int q = j; q < b; q += 64) {
    u0 += work[3 * q + 0];
    n0 += work[3 * q + 1];
  }
  if (last)
    for (int q = j; q < B; q += 64) bad += work[3 * q + 2];
  u0 = wave_sum_i(u0);
  n0 = wave_sum_i(n0);
  const PlanSlot s = plan_slot(pos, labels, weights, valid_len, b, P, L, V, s_pos, s_first);
  if (s.entry) {
    const int e = n0 + s.rank;
    out_labels[e] = s.label;
    out_weights[e] = s.w;
    out_sample[e] = b;
    if (s.first) {
      rows[u0 + s.row] = b * L + s.pos;
      row_ptr[u0 + s.row] = e;                                      // the first slot of a row is its first entry
    }
  }
  if (last) {
    bad = wave_sum_i(bad);
    if (j == 0) {
      const int U = u0 + work[3 * b + 0], n = n0 + work[3 * b + 1];
      row_ptr[U] = n;
      counts[0] = U;
      counts[1] = n;
      counts[2] = bad;
      counts[3] = 0;
    }
  }
}

}  // namespace

extern "C" int mv_report_draws(unsigned long long key, unsigned long long step, int B, int T, uint32_t* draws, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!draws || B <= 0 || T <= 0) return MV_E_ARG;
  if (T > MAX_T || (long long)B * (T + 1) > 0x3fffffffLL) return MV_E_SHAPE;          // LDS words; 32-bit hash counters
  unsigned k0, k1;
  mv_derive_keys(key, step, k0, k1);
  const int n = B * (T + 1);
  report_draws_kernel<<<(n + 255) / 256, 256, 0, stream>>>(k0, k1, n, draws);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_report_assemble(const int64_t* txt_ids, const int32_t* txt_len, const int32_t* n_pred, int n_items, const void* img_feats,
                                  int dtype, const int64_t* img_pos, const int32_t* idx, const int32_t* family, int B, int N, int T, int F,
                                  int max_pred, unsigned long long key, unsigned long long step, const uint32_t* draws,
                                  int64_t* input_txt, int64_t* segment, int32_t* desc, void* feats, int64_t* pos_out,
                                  int64_t* masked_pos, int64_t* masked_lm_labels, float* masked_weights, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!txt_ids || !txt_len || !n_pred || !img_feats || !img_pos || !idx || !input_txt || !segment || !desc || !feats || !pos_out ||
      !masked_pos || !masked_lm_labels || !masked_weights)
    return MV_E_ARG;
  if (n_items <= 0 || B <= 0 || N <= 0 || T <= 0 || F <= 0 || max_pred <= 0) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if (T > MAX_T || max_pred > MAX_PRED) return MV_E_SHAPE;
  if ((long long)N * F > 0x7fffffffLL || (long long)B * (T + 1) > 0x3fffffffLL) return MV_E_SHAPE;
  unsigned k0, k1;
  mv_derive_keys(key, step, k0, k1);
  typedef mv_types<float, bf16_t, f16_t> Accept;      // f16 runs the bf16 instantiation: 2-byte elements move as bits (mv_bits_t)
  return mv_with_type(dtype, Accept{}, [&](auto t) -> int {
    typedef mv_bits_t<MV_T(t)> E;
    const ChunkPlan p = chunk_plan((unsigned)((long long)N * F), sizeof(E), img_feats, feats);
    hipLaunchKernelGGL(report_assemble_kernel<E>, dim3((unsigned)B, p.chunks), dim3(NT), 0, stream, txt_ids, txt_len, n_pred, n_items,
                       (const E*)img_feats, img_pos, idx, family, N, T, max_pred, k0, k1, draws, input_txt, segment, desc, (E*)feats, pos_out,
                       masked_pos, masked_lm_labels, masked_weights, p);
    return (int)hipGetLastError();
  });
}

extern "C" int mv_report_plan(const int64_t* pos, const int64_t* labels, const float* weights, const int32_t* valid_len, int B, int P, int L,
                              int V, int32_t* work, int32_t* rows, int32_t* row_ptr, int32_t* out_labels, float* out_weights,
                              int32_t* out_sample, int32_t* counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!pos || !labels || !weights || !work || !rows || !row_ptr || !out_labels || !out_weights || !out_sample || !counts) return MV_E_ARG;
  if (B <= 0 || P <= 0 || L <= 0 || V <= 0) return MV_E_ARG;
  if (P > MAX_PRED || B > PLAN_MAX_B || (long long)B * L > 0x7fffffffLL) return MV_E_SHAPE;      // one wave per sample; int32 flat rows
  report_plan_count_kernel<<<B, 64, 0, stream>>>(pos, labels, weights, valid_len, P, L, V, work);
  MV_CHECK_LAUNCH();
  report_plan_write_kernel<<<B, 64, 0, stream>>>(pos, labels, weights, valid_len, B, P, L, V, work, rows, row_ptr, out_labels, out_weights,
                                                 out_sample, counts);
  MV_CHECK_LAUNCH();
  return MV_OK;
}
