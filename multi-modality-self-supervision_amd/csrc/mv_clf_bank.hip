// Diagnosis classification from a device-resident bank (the reference's JsonlDataset + collate_fn, Downstream_task/Classification/mmbt/
// data/dataset.py:36-85 and data/helpers.py:73-98, and the metrics of model_eval, mmbt/main.py:138-193):
//   mv_clf_assemble  one launch per batch: the text rows, segment, mask descriptors, the gathered region features of each sample's image
//                    and the dense multi-hot target from the packed label bits
//   mv_clf_counts    a whole evaluation's sigmoid probabilities -> the integer counts AUROC and F1 follow from, per class and over all
//                    (sample, class) elements as one list
// Integer and copy work.  mv_clf_assemble accumulates nothing: the same input gives the same bits on every run.  mv_clf_counts counts in
// integers and adds each block's counts with 64-bit integer atomics: its sums do not depend on the order in which blocks finish.
#include "mv_bank.h"

namespace {
using namespace mv_bank;

constexpr int MAX_T = 1024;           // text ids per row
constexpr int MAX_C = 1024;           // classes
constexpr int FAMILY_1D = 4;
constexpr int MAX_ELEMS = 2097152;    // n C of mv_clf_counts: pair counting is quadratic
constexpr int RPT = 8;                // elements of the negative side a lane holds in registers
constexpr int TILE = 2048;            // NT RPT: the negative side of a block; also the candidates of one round of the positive side
constexpr int NCOUNT = 7;             // n_pos, n_neg, gt, eq, tp, fp, fn
constexpr int SPLIT_BLOCKS = 2048;    // the positive side is split over blocks until a list has about this many

struct ClfBankArgs {                  // the bank, as mv_clf_assemble reads it
  const int64_t* txt_ids;
  const int32_t* txt_len;
  const int32_t* s_img;
  const int32_t* lab_bits;
  const int64_t* img_pos;
  int n_samples, n_images;
};

// class c of sample d: bit c % 32 of word c / 32
__device__ __forceinline__ int label_bit(const int32_t* __restrict__ lab_bits, int d, int W, int c) {
  return ((unsigned)lab_bits[(size_t)d * W + (c >> 5)] >> (c & 31)) & 1u;
}

// grid (B, chunks): every block of a sample copies one chunk of its image's feature row; chunk 0 also writes the sample's small outputs.
template <typename T>
__global__ __launch_bounds__(NT) void clf_assemble_kernel(ClfBankArgs bk, const T* __restrict__ img, const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ family, int N, int Tn, int C,
                                                          int64_t* __restrict__ input_txt, int64_t* __restrict__ segment,
                                                          int32_t* __restrict__ desc, T* __restrict__ feats, int64_t* __restrict__ pos_out,
                                                          float* __restrict__ target, ChunkPlan plan) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int d = clamp_item(idx[i], bk.n_samples);
  const int m = clamp_item(bk.s_img[d], bk.n_images);
  if (blockIdx.y == 0) {
    const int len = min(max(bk.txt_len[d], 1), Tn);
    const int64_t* src = bk.txt_ids + (size_t)d * Tn;
    for (int t = tid; t < Tn; t += NT) {
      input_txt[(size_t)i * Tn + t] = src[t];
      segment[(size_t)i * Tn + t] = t < len ? 1 : 0;               // dataset.py:83, zero over the padding (helpers.py:79,95)
    }
    copy_pos_row(bk.img_pos, m, pos_out, i, N);
    const int W = (C + 31) >> 5;
    for (int c = tid; c < C; c += NT) target[(size_t)i * C + c] = label_bit(bk.lab_bits, d, W, c) ? 1.f : 0.f;
    if (tid == 0) write_desc(desc, i, family ? family[i] : FAMILY_1D, N, len);
  }
  copy_chunk(img + (size_t)m * plan.row, feats + (size_t)i * plan.row, plan.row, blockIdx.y * plan.chunk, plan.chunk, plan.vec);
}

// ---- mv_clf_counts
// An order-preserving key of a probability in [1, 0xFFFFFFFE]: a < b <=> key(a) < key(b) and a == b <=> key(a) == key(b) for every pair
// of non-NaN floats (-0 is taken as +0).  0 and 0xFFFFFFFF stay free for the elements that count nothing.
__device__ __forceinline__ unsigned prob_key(float p) {
  unsigned b = __float_as_uint(p);
  if (b == 0x80000000u) b = 0u;
  const unsigned k = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  return min(k, 0xFFFFFFFDu) + 1u;
}
constexpr unsigned KEY_NO_NEG = 0xFFFFFFFFu;      // in a register: no positive's key is above or equal
constexpr unsigned KEY_NO_POS = 0u;               // in LDS: above or equal to no negative's key

// element e of list z: class z's list holds the n samples, list C every (sample, class) element in row-major order
__device__ __forceinline__ void list_elem(int z, int C, unsigned e, int& j, int& c) {
  if (z < C) {
    j = (int)e;
    c = z;
  } else {
    j = (int)(e / (unsigned)C);
    c = (int)(e - (unsigned)j * (unsigned)C);
  }
}

// grid (tiles of the negative side, splits of the positive side, C + 1 lists).  A block holds TILE elements of its list in registers as
// negatives (a positive or an element past the list: KEY_NO_NEG), walks its share of the list in rounds of TILE candidates whose positives
// it packs into LDS, and compares every packed positive (one broadcast read for four) with its RPT registers, branch-free.  The blocks of
// split 0 also count their tile's n_pos, n_neg, tp, fp, fn.
__global__ __launch_bounds__(NT) void clf_counts_kernel(const float* __restrict__ probs, int ld, const int32_t* __restrict__ idx, int n,
                                                        const int32_t* __restrict__ lab_bits, int n_items, int C, unsigned span,
                                                        unsigned long long* __restrict__ counters) {
  __shared__ __attribute__((aligned(16))) unsigned s_key[TILE + 4];
  __shared__ unsigned s_cnt;
  __shared__ unsigned long long s_red[NT / 64];
  const int tid = threadIdx.x, z = blockIdx.z;
  const unsigned len = z < C ? (unsigned)n : (unsigned)n * (unsigned)C;
  const unsigned t0 = blockIdx.x * (unsigned)TILE;
  const unsigned lo = blockIdx.y * span, hi = min(len, lo + span);
  if (t0 >= len || lo >= len) return;                               // (uniform over the block)
  const int W = (C + 31) >> 5;

  unsigned q[RPT];
  unsigned n_pos = 0, n_neg = 0, tp = 0, fp = 0, fn = 0;
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const unsigned e = t0 + r * NT + tid;
    q[r] = KEY_NO_NEG;
    if (e < len) {
      int j, c;
      list_elem(z, C, e, j, c);
      const float p = probs[(size_t)j * ld + c];
      const int y = label_bit(lab_bits, clamp_item(idx[j], n_items), W, c);
      const int hit = p > 0.5f;                                     // the reference's threshold (main.py:148)
      if (!y) q[r] = prob_key(p);
      n_pos += y;
      n_neg += !y;
      tp += hit & y;
      fp += hit & !y;
      fn += !hit & y;
    }
  }

  unsigned gt = 0, eq = 0;
  for (unsigned base = lo; base < hi; base += TILE) {
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int r = 0; r < RPT; ++r) {
      const unsigned e = base + r * NT + tid;
      if (e < hi) {
        int j, c;
        list_elem(z, C, e, j, c);
        if (label_bit(lab_bits, clamp_item(idx[j], n_items), W, c))
          s_key[atomicAdd(&s_cnt, 1u)] = prob_key(probs[(size_t)j * ld + c]);      // (the order inside LDS changes no count)
      }
    }
    __syncthreads();
    const unsigned cnt = s_cnt, cnt4 = (cnt + 3u) & ~3u;
    if (tid < (int)(cnt4 - cnt)) s_key[cnt + tid] = KEY_NO_POS;
    __syncthreads();
    for (unsigned k = 0; k < cnt4; k += 4) {
      const uint4 p = *(const uint4*)&s_key[k];
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        gt += (p.x > q[r]) + (p.y > q[r]) + (p.z > q[r]) + (p.w > q[r]);
        eq += (p.x == q[r]) + (p.y == q[r]) + (p.z == q[r]) + (p.w == q[r]);
      }
    }
    __syncthreads();                                                // (the next round rewrites s_key and s_cnt)
  }

  unsigned long long* row = counters + (size_t)z * NCOUNT;
  block_add(gt, row + 2, s_red);
  block_add(eq, row + 3, s_red);
  if (blockIdx.y == 0) {
    block_add(n_pos, row + 0, s_red);
    block_add(n_neg, row + 1, s_red);
    block_add(tp, row + 4, s_red);
    block_add(fp, row + 5, s_red);
    block_add(fn, row + 6, s_red);
  }
}

}  // namespace

extern "C" int mv_clf_assemble(const int64_t* txt_ids, const int32_t* txt_len, const int32_t* s_img, const int32_t* lab_bits, int n_samples,
                               const void* img_feats, int dtype, const int64_t* img_pos, int n_images, const int32_t* idx,
                               const int32_t* family, int B, int N, int T, int F, int C, int64_t* input_txt, int64_t* segment, int32_t* desc,
                               void* feats, int64_t* pos_out, float* target, void* stream_) {
  typedef mv_types<float, bf16_t, f16_t> Accept;      // f16 runs the bf16 instantiation: 2-byte elements move as bits (mv_bits_t)
  hipStream_t stream = (hipStream_t)stream_;
  if (!txt_ids || !txt_len || !s_img || !lab_bits || !img_feats || !img_pos || !idx || !input_txt || !segment || !desc || !feats ||
      !pos_out || !target)
    return MV_E_ARG;
  if (n_samples <= 0 || n_images <= 0 || B <= 0 || N <= 0 || T <= 0 || F <= 0 || C <= 0) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if (T > MAX_T || C > MAX_C || (long long)N * F > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL) return MV_E_SHAPE;
  const ClfBankArgs bk = {txt_ids, txt_len, s_img, lab_bits, img_pos, n_samples, n_images};
  return mv_with_type(dtype, Accept{}, [&](auto t) -> int {
    typedef mv_bits_t<MV_T(t)> E;
    const ChunkPlan p = chunk_plan((unsigned)((long long)N * F), sizeof(E), img_feats, feats);
    hipLaunchKernelGGL(clf_assemble_kernel<E>, dim3((unsigned)B, p.chunks), dim3(NT), 0, stream, bk, (const E*)img_feats, idx, family, N, T,
                       C, input_txt, segment, desc, (E*)feats, pos_out, target, p);
    return (int)hipGetLastError();
  });
}

extern "C" int mv_clf_counts(const float* probs, int ld, const int32_t* idx, int n, const int32_t* lab_bits, int n_items, int C,
                             unsigned long long* counters, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!probs || !idx || !lab_bits || !counters) return MV_E_ARG;
  if (n <= 0 || n_items <= 0 || C <= 0 || ld < C) return MV_E_ARG;
  if (C > MAX_C || (long long)n * C > MAX_ELEMS) return MV_E_SHAPE;
  static_assert(TILE == NT * RPT, "a block's tile is RPT elements per lane");
  const unsigned tiles = ((unsigned)n * (unsigned)C + TILE - 1) / TILE;             // of the longest list
  const unsigned want = (unsigned)SPLIT_BLOCKS / tiles;
  const unsigned splits = want < 1u ? 1u : (want < tiles ? want : tiles);
  const unsigned span = (tiles + splits - 1) / splits * TILE;                       // whole rounds
  clf_counts_kernel<<<dim3(tiles, (tiles * TILE + span - 1) / span, (unsigned)C + 1), NT, 0, stream>>>(probs, ld, idx, n, lab_bits, n_items,
                                                                                                      C, span, counters);
  MV_CHECK_LAUNCH();
  return MV_OK;
}
