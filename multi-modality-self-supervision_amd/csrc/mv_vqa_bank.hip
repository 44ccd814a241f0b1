// VQA fine-tuning and evaluation from a device-resident question bank (the reference's VQA-RAD loader, Downstream_task/
// report_generation_and_vqa/sc/data_loader.py:236-273, its Preprocess4Seq2seq for questions, :340-392, and the score of
// pytorch_pretrained_bert/model.py:1007-1023):
//   mv_vqa_assemble  one launch per batch: the question rows, segment, mask descriptors, the gathered region features of each question's
//                    image, the dense soft target from the sparse answers and the answer types
//   mv_vqa_score     the score of a batch of predicted answer columns, and the integer sums of a whole evaluation by (group, type)
// Integer and copy work.  mv_vqa_assemble accumulates nothing: the same input gives the same bits on every run.  mv_vqa_score adds
// 32.32 fixed-point terms with 64-bit integer atomics, so its sums do not depend on the order in which samples finish either.
#include "mv_bank.h"

namespace {
using namespace mv_bank;

constexpr int MAX_T = 1024;           // text ids per row
constexpr int MAX_G = 8;              // groups of mv_vqa_score
constexpr int FAMILY_1D = 4;

struct VqaBankArgs {                  // the bank, as mv_vqa_assemble reads it
  const int64_t* txt_ids;
  const int32_t* txt_len;
  const int32_t* q_img;
  const int32_t* ans_ptr;
  const int32_t* ans_label;
  const float* ans_score;
  const int32_t* ans_type;
  const int64_t* img_pos;
  int n_questions, n_images, nnz;
};

// grid (B, chunks): every block of a sample copies one chunk of its image's feature row; chunk 0 also writes the sample's small outputs.
template <typename T>
__global__ __launch_bounds__(NT) void vqa_assemble_kernel(VqaBankArgs bk, const T* __restrict__ img, const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ family, int N, int Tn, int A,
                                                          int64_t* __restrict__ input_txt, int64_t* __restrict__ segment,
                                                          int32_t* __restrict__ desc, T* __restrict__ feats, int64_t* __restrict__ pos_out,
                                                          float* __restrict__ target, int32_t* __restrict__ ans_type_out, ChunkPlan plan) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int d = clamp_item(idx[i], bk.n_questions);
  const int m = clamp_item(bk.q_img[d], bk.n_images);
  if (blockIdx.y == 0) {
    const int len = min(max(bk.txt_len[d], 1), Tn);
    const int64_t* src = bk.txt_ids + (size_t)d * Tn;
    for (int t = tid; t < Tn; t += NT) {
      input_txt[(size_t)i * Tn + t] = src[t];                       // unmasked: VQA predicts no token (data_loader.py:378-381)
      segment[(size_t)i * Tn + t] = t < len ? 1 : 0;
    }
    copy_pos_row(bk.img_pos, m, pos_out, i, N);
    float* trow = target + (size_t)i * A;
    for (int a = tid; a < A; a += NT) trow[a] = 0.f;
    if (tid == 0) {
      write_desc(desc, i, family ? family[i] : FAMILY_1D, N, len);
      ans_type_out[i] = bk.ans_type[d];
    }
    __syncthreads();                                                // (the block's own zeros are ordered before the entries below)
    if (tid == 0) {
      const int e0 = min(max(bk.ans_ptr[d], 0), bk.nnz), e1 = min(max(bk.ans_ptr[d + 1], e0), bk.nnz);
      for (int e = e0; e < e1; ++e) {                               // CSR order: a later duplicate of a label wins, as scatter_ on the CPU
        const int l = bk.ans_label[e];
        if (l >= 0 && l < A) trow[l] = bk.ans_score[e];
      }
    }
  }
  copy_chunk(img + (size_t)m * plan.row, feats + (size_t)i * plan.row, plan.row, blockIdx.y * plan.chunk, plan.chunk, plan.vec);
}

// 32.32 fixed point of a score, rounded to nearest even (mv_rank_groups' device): integer sums do not depend on the order of the samples.
// A negative score is added in two's complement.
__device__ __forceinline__ unsigned long long score_fx(float s) { return (unsigned long long)(long long)rint(ldexp((double)s, 32)); }

// one lane per sample
__global__ __launch_bounds__(NT) void vqa_score_kernel(const int64_t* __restrict__ pred, const int32_t* __restrict__ idx, int B,
                                                       int n_questions, const int32_t* __restrict__ ans_ptr,
                                                       const int32_t* __restrict__ ans_label, const float* __restrict__ ans_score, int nnz,
                                                       const int32_t* __restrict__ ans_type, const int32_t* __restrict__ group, int G,
                                                       float* __restrict__ score, unsigned long long* __restrict__ counters) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= B) return;
  const int d = min(max(idx[i], 0), n_questions - 1);
  const int64_t p = pred[i];
  const int e0 = min(max(ans_ptr[d], 0), nnz), e1 = min(max(ans_ptr[d + 1], e0), nnz);
  float s = 0.f;
  for (int e = e0; e < e1; ++e)
    if ((int64_t)ans_label[e] == p) s = ans_score[e];               // the last entry of the label: what the dense target holds
  if (score) score[i] = s;
  const int ty = ans_type[d];
  const int slot = ty == 0 ? 0 : (ty == 1 ? 1 : 2);                 // closed, open, neither
  const int g = group ? min(max(group[d], 0), G - 1) : 0;
  unsigned long long* c = counters + ((size_t)g * 3 + slot) * 2;
  atomicAdd(c, score_fx(s));
  atomicAdd(c + 1, 1ull);
}

}  // namespace

extern "C" int mv_vqa_assemble(const int64_t* txt_ids, const int32_t* txt_len, const int32_t* q_img, int n_questions,
                               const int32_t* ans_ptr, const int32_t* ans_label, const float* ans_score, int nnz, const int32_t* ans_type,
                               const void* img_feats, int dtype, const int64_t* img_pos, int n_images, const int32_t* idx,
                               const int32_t* family, int B, int N, int T, int F, int A, int64_t* input_txt, int64_t* segment,
                               int32_t* desc, void* feats, int64_t* pos_out, float* target, int32_t* ans_type_out, void* stream_) {
  typedef mv_types<float, bf16_t, f16_t> Accept;      // f16 runs the bf16 instantiation: 2-byte elements move as bits (mv_bits_t)
  hipStream_t stream = (hipStream_t)stream_;
  if (!txt_ids || !txt_len || !q_img || !ans_ptr || !ans_type || !img_feats || !img_pos || !idx || !input_txt || !segment || !desc ||
      !feats || !pos_out || !target || !ans_type_out)
    return MV_E_ARG;
  if (n_questions <= 0 || n_images <= 0 || B <= 0 || N <= 0 || T <= 0 || F <= 0 || A <= 0 || nnz < 0) return MV_E_ARG;
  if (nnz > 0 && (!ans_label || !ans_score)) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if (T > MAX_T || (long long)N * F > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL) return MV_E_SHAPE;
  const VqaBankArgs bk = {txt_ids, txt_len, q_img, ans_ptr, ans_label, ans_score, ans_type, img_pos, n_questions, n_images, nnz};
  return mv_with_type(dtype, Accept{}, [&](auto t) -> int {
    typedef mv_bits_t<MV_T(t)> E;
    const ChunkPlan p = chunk_plan((unsigned)((long long)N * F), sizeof(E), img_feats, feats);
    hipLaunchKernelGGL(vqa_assemble_kernel<E>, dim3((unsigned)B, p.chunks), dim3(NT), 0, stream, bk, (const E*)img_feats, idx, family, N, T,
                       A, input_txt, segment, desc, (E*)feats, pos_out, target, ans_type_out, p);
    return (int)hipGetLastError();
  });
}

extern "C" int mv_vqa_score(const int64_t* pred, const int32_t* idx, int B, int n_questions, const int32_t* ans_ptr,
                            const int32_t* ans_label, const float* ans_score, int nnz, const int32_t* ans_type, const int32_t* group, int G,
                            float* score, unsigned long long* counters, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!pred || !idx || !ans_ptr || !ans_type || !counters) return MV_E_ARG;
  if (B <= 0 || n_questions <= 0 || G <= 0 || nnz < 0) return MV_E_ARG;
  if (nnz > 0 && (!ans_label || !ans_score)) return MV_E_ARG;
  if (G > MAX_G) return MV_E_SHAPE;
  vqa_score_kernel<<<(B + NT - 1) / NT, NT, 0, stream>>>(pred, idx, B, n_questions, ans_ptr, ans_label, ans_score, nnz, ans_type, group, G,
                                                          score, counters);
  MV_CHECK_LAUNCH();
  return MV_OK;
}
