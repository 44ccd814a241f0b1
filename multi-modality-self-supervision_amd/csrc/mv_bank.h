// What the batch kernels of the device-resident banks share (mv_pair_assemble, mv_report_assemble, mv_vqa_assemble): each launches a
// grid (samples, chunks) in which every block copies one chunk of its sample's feature row out of the image bank -- the gather all
// three are HBM-bound on -- and chunk 0 also writes the sample's small outputs.  Here: the copy, the launcher's chunk plan and the
// pieces of chunk 0 that do not depend on the task.  The text side of each kernel stays in its own file.  Also the block sum into a
// 64-bit counter that the kernels behind the evaluations' metrics share.
#pragma once
#include "mv_dispatch.h"

namespace mv_bank {

constexpr int NT = 256;               // threads of an assemble block
constexpr int VEC_BYTES = 16;         // one lane's load / store on the aligned path
constexpr int UNROLL = 4;             // vectors a lane holds in flight
constexpr int CHUNK_BYTES = 65536;    // one block's share of a feature row
constexpr int MAX_CHUNKS = 1024;      // blocks per sample: longer rows take larger chunks

// One block's share of a feature row: elements [lo, min(n, lo + chunk)) of s -> d.  vec: n, chunk and both bases are multiples of 16
// bytes -> 16 bytes per lane, UNROLL loads issued before the first store; else element by element.
template <typename T>
__device__ __forceinline__ void copy_chunk(const T* __restrict__ s, T* __restrict__ d, unsigned n, unsigned lo, unsigned chunk, int vec) {
  if (lo >= n) return;
  const unsigned cnt = min(n - lo, chunk);
  if (vec) {
    const uint4* s4 = (const uint4*)(s + lo);
    uint4* d4 = (uint4*)(d + lo);
    const unsigned n4 = cnt / (VEC_BYTES / sizeof(T));
    const unsigned body = n4 / (UNROLL * NT) * (UNROLL * NT);
    for (unsigned i = threadIdx.x; i < body; i += UNROLL * NT) {
      uint4 v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = s4[i + u * NT];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) d4[i + u * NT] = v[u];
    }
    for (unsigned i = body + threadIdx.x; i < n4; i += NT) d4[i] = s4[i];
  } else {
    for (unsigned i = threadIdx.x; i < cnt; i += NT) d[lo + i] = s[lo + i];
  }
}

// The launcher's side of copy_chunk for rows of `row` elements of `elem` bytes: grid (samples, chunks), block y copies the elements from
// y * chunk on; the kernel is handed the plan.  src / dst: the bases of the bank and of the gathered batch (every row starts a whole
// number of rows behind them).
struct ChunkPlan {
  unsigned row, chunk, chunks;
  int vec;
};
inline ChunkPlan chunk_plan(unsigned row, unsigned elem, const void* src, const void* dst) {
  const unsigned per_vec = VEC_BYTES / elem;
  ChunkPlan p;
  p.row = row;
  p.chunk = CHUNK_BYTES / elem;
  p.chunks = (row + p.chunk - 1) / p.chunk;
  if (p.chunks > MAX_CHUNKS) {                           // bound the grid's second dimension: larger chunks, still whole vectors
    p.chunk = ((row + MAX_CHUNKS - 1) / MAX_CHUNKS + per_vec - 1) / per_vec * per_vec;
    p.chunks = (row + p.chunk - 1) / p.chunk;
  }
  p.vec = (row % per_vec == 0 && ((uintptr_t)src % VEC_BYTES) == 0 && ((uintptr_t)dst % VEC_BYTES) == 0) ? 1 : 0;
  return p;
}

// ---- chunk 0: the small outputs every task writes the same way
// an index outside its bank of n items is clamped: it reads no foreign memory
__device__ __forceinline__ int clamp_item(int v, int n) { return min(max(v, 0), n - 1); }

// sample i takes the position row of image m (mv_pair_assemble hands over a null pair when the bank has no positions)
__device__ __forceinline__ void copy_pos_row(const int64_t* __restrict__ img_pos, int m, int64_t* __restrict__ pos_out, int i, int N) {
  if (!img_pos) return;
  for (int j = threadIdx.x; j < N; j += NT) pos_out[(size_t)i * N + j] = img_pos[(size_t)m * N + j];
}

// the mask descriptor of sample i: N regions between [CLS] and [SEP], then len valid text positions (one lane writes it)
__device__ __forceinline__ void write_desc(int32_t* __restrict__ desc, int i, int family, int N, int len) {
  desc[3 * i + 0] = family;
  desc[3 * i + 1] = N + 2;
  desc[3 * i + 2] = N + 2 + len;
}

// ---- the counting kernels (mv_clf_counts, mv_bleu_counts)
// the block's sum of v -> one 64-bit atomic (none for a zero); every lane of the NT calls it, sh holds NT / 64 words
__device__ __forceinline__ void block_add(unsigned long long v, unsigned long long* __restrict__ dst, unsigned long long* sh) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < NT / 64; ++w) t += sh[w];
    if (t) atomicAdd(dst, t);
  }
  __syncthreads();
}

}  // namespace mv_bank
