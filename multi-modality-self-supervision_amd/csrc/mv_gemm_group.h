// Grouped weight-gradient launch (mv_gemm_grouped_tn): the table of problems, the unit -> (problem, tile, K-slice) map and the
// tail rule.  Plain C++ shared by the host (mv_gemm.hip builds and checks the table; tests/native/group_plan_check.cpp drives
// it under the host sanitizers) and by the kernels (mv_gemm_ring.h decodes a unit with the SAME function), so there is one
// definition of the map.
//
// Every problem is C[No, Ko] (+)= alpha * A[rows, No]^T . B[rows, Ko] on 256 x 256 tiles.  All tiles of all problems form ONE flat
// list of full-K units (problem after problem).  With U units and G blocks (one per CU):
//   * the first floor(U / G) * G units run unsplit and write C directly;
//   * the remaining R = U mod G units are cut along K by the smallest factor s <= MV_GROUP_MAX_SPLIT whose R * s units fill the
//     rounds they occupy to at least 70 % (R * s >= 0.7 * ceil(R * s / G) * G); s = 1 (also when no factor reaches 70 %) keeps them
//     unsplit.  Split units write f32 slabs ([tail tile][slice][256][256]) that ONE reduction launch folds into C.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/medvill.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MV_HD __host__ __device__ __forceinline__
#else
#define MV_HD inline
#endif

#define MV_GROUP_MAGIC 0x4d564754     // "MVGT"
#define MV_GROUP_MAX_PROBLEMS 256
#define MV_GROUP_MAX_SPLIT 8
#define MV_GROUP_TILE 256
#define MV_GROUP_BK 64                // contraction depth of one ring stage: slices are multiples of it

struct MvGroupHeader {                // 64 bytes
  int magic, count, dtype, n_blocks;  // n_blocks = G the plan was made for
  int units;                          // U: 256 x 256 tiles of all problems
  int direct;                         // units [0, direct) run unsplit
  int tail;                           // tiles [direct, units) are split ...
  int split;                          // ... `split` ways (1: tail == 0)
  int pad[8];
};
struct MvGroupEntry {                 // 64 bytes, one per problem
  const void* A; const void* B; void* C;
  int lda, ldb, ldc;
  int M, N, K;                        // No, Ko, rows
  unsigned bytesA, bytesB;            // sizes of the operands' buffer resources (< 2 GiB)
  int unit0;                          // first flat unit (tile) of this problem
  int kchunk;                         // K-slice depth of this problem's split tiles (multiple of MV_GROUP_BK; K when nothing splits)
};
struct GroupArgs {                    // what the kernels of a grouped launch receive
  const void* table;                  // device copy of the table: MvGroupHeader, then the entries
  float* ws;                          // slabs of the tail tiles: [tail tile][slice][256][256]
  const float* alpha;
  int accumulate;
};
static_assert(sizeof(MvGroupHeader) == 64 && sizeof(MvGroupEntry) == 64, "table layout");

MV_HD int mv_group_tiles(int M, int N) { return ((M + MV_GROUP_TILE - 1) / MV_GROUP_TILE) * ((N + MV_GROUP_TILE - 1) / MV_GROUP_TILE); }

// the tail rule: split factor of the R units that do not fill a round of G blocks
MV_HD int mv_group_tail_split(int R, int G) {
  if (R <= 0 || G <= 0) return 1;
  for (int s = 1; s <= MV_GROUP_MAX_SPLIT; ++s) {
    const long long n = (long long)R * s, rounds = (n + G - 1) / G;
    if (10 * n >= 7 * rounds * G) return s;
  }
  return 1;
}

// a bijection of [0, n): the 8 XCDs (blocks b, b + 8, ... share an L2; unit u runs on block u mod G) each take a contiguous run
MV_HD int mv_group_xcd_remap(int u, int n) {
  const int q = n >> 3, r = n & 7, xcd = u & 7, in = u >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + in;
}

// 8-row grouped raster inside one problem: tile t -> (m0, n0)
MV_HD void mv_group_raster(int t, int M, int N, int& m0, int& n0) {
  const int tiles_n = (N + MV_GROUP_TILE - 1) / MV_GROUP_TILE, tiles_m = (M + MV_GROUP_TILE - 1) / MV_GROUP_TILE;
  const int GM = 8, per_group = GM * tiles_n;
  const int group = t / per_group, rem = t - group * per_group;
  const int gm = (tiles_m - group * GM) < GM ? (tiles_m - group * GM) : GM;
  m0 = (group * GM + rem % gm) * MV_GROUP_TILE;
  n0 = (rem / gm) * MV_GROUP_TILE;
}

// problem that owns flat tile `t` (entries are sorted by unit0; 0 <= t < units)
template <typename EP>
MV_HD int mv_group_find(EP e, int count, int t) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (e[mid].unit0 <= t) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct MvGroupUnit {
  int problem, tile;      // tile: flat tile index
  int m0, n0, kbeg, kend;
  int slice;              // -1: unsplit, the unit writes C; else the K-slice, the unit writes slab (tile - direct) * split + slice
};
// launch unit u in [0, direct + tail * split) -> what it computes.  Units that run together on one XCD are neighbouring tiles of
// one problem (and of one slice).
template <typename EP>       // EP: pointer to the entries (the kernels pass a constant-address-space pointer: scalar loads)
MV_HD MvGroupUnit mv_group_decode(const MvGroupHeader& h, EP e, int u) {
  MvGroupUnit d;
  if (u < h.direct) {
    d.tile = mv_group_xcd_remap(u, h.direct);
    d.slice = -1;
  } else {
    const int v = mv_group_xcd_remap(u - h.direct, h.tail * h.split);
    d.slice = v / h.tail;
    d.tile = h.direct + (v - d.slice * h.tail);
  }
  d.problem = mv_group_find(e, h.count, d.tile);
  const int pM = e[d.problem].M, pN = e[d.problem].N, pK = e[d.problem].K, kc = e[d.problem].kchunk;
  mv_group_raster(d.tile - e[d.problem].unit0, pM, pN, d.m0, d.n0);
  if (d.slice < 0) { d.kbeg = 0; d.kend = pK; }
  else {      // a slice past the end of a short contraction is empty (kend == kbeg): its slab is written as zeros
    const long long kb = (long long)d.slice * kc;
    d.kbeg = kb < pK ? (int)kb : pK;
    d.kend = (kb + kc) < pK ? (int)(kb + kc) : pK;
  }
  return d;
}

#ifndef MV_GROUP_DEVICE_ONLY
// ---- host: the caller's problem list (include/medvill.h: mv_group_problem) -> table.  Returns an MV_E_* code; writes nothing on failure.
typedef mv_group_problem MvGroupProblemIn;

inline int mv_group_check_problem(const MvGroupProblemIn& q) {
  if (!q.A || !q.B || !q.C || q.No <= 0 || q.Ko <= 0 || q.rows <= 0) return MV_E_ARG;
  if (q.lda < q.No || q.ldb < q.Ko || q.ldc < q.Ko) return MV_E_SHAPE;
  if ((q.lda & 7) || (q.ldb & 7) || (((uintptr_t)q.A) & 15) || (((uintptr_t)q.B) & 15) || (((uintptr_t)q.C) & 3)) return MV_E_SHAPE;
  const unsigned long long bA = ((unsigned long long)(q.rows - 1) * q.lda + (unsigned long long)((q.No + 7) & ~7)) * 2;
  const unsigned long long bB = ((unsigned long long)(q.rows - 1) * q.ldb + (unsigned long long)((q.Ko + 7) & ~7)) * 2;
  const unsigned long long bC = ((unsigned long long)(q.No - 1) * q.ldc + (unsigned long long)q.Ko) * 4;
  if (bA >= 0x7fffffffULL || bB >= 0x7fffffffULL || bC >= 0x7fffffffULL) return MV_E_SHAPE;
  return 0;
}

// size of an operand's buffer resource: the last row ends with its width rounded up to the 16-byte pieces the DMA reads
inline unsigned mv_group_operand_bytes(int rows, int ld, int width) {
  return (unsigned)(((unsigned long long)(rows - 1) * ld + (unsigned long long)((width + 7) & ~7)) * 2);
}

inline size_t mv_group_table_bytes(int count) { return count > 0 ? sizeof(MvGroupHeader) + (size_t)count * sizeof(MvGroupEntry) : 0; }

inline int mv_group_fill(int dtype, int count, const MvGroupProblemIn* probs, int n_blocks, void* table, size_t table_bytes) {
  if (!probs || !table || count <= 0 || n_blocks <= 0) return MV_E_ARG;
  if (dtype != MV_BF16 && dtype != MV_F16) return MV_E_DTYPE;       // 16-bit operands
  if (count > MV_GROUP_MAX_PROBLEMS) return MV_E_SHAPE;
  if (table_bytes < mv_group_table_bytes(count)) return MV_E_WORKSPACE;
  long long units = 0;
  for (int i = 0; i < count; ++i) {
    const int rc = mv_group_check_problem(probs[i]);
    if (rc) return rc;
    units += mv_group_tiles(probs[i].No, probs[i].Ko);
  }
  if (units > (1 << 24)) return MV_E_SHAPE;
  MvGroupHeader h = {};
  h.magic = MV_GROUP_MAGIC; h.count = count; h.dtype = dtype; h.n_blocks = n_blocks; h.units = (int)units;
  const int rem = (int)(units % n_blocks);
  h.split = mv_group_tail_split(rem, n_blocks);
  h.tail = h.split > 1 ? rem : 0;
  h.direct = h.units - h.tail;
  MvGroupEntry* e = (MvGroupEntry*)((char*)table + sizeof(MvGroupHeader));
  int u0 = 0;
  for (int i = 0; i < count; ++i) {
    const MvGroupProblemIn& q = probs[i];
    MvGroupEntry& t = e[i];
    t.A = q.A; t.B = q.B; t.C = q.C; t.lda = q.lda; t.ldb = q.ldb; t.ldc = q.ldc; t.M = q.No; t.N = q.Ko; t.K = q.rows;
    t.bytesA = mv_group_operand_bytes(q.rows, q.lda, q.No);
    t.bytesB = mv_group_operand_bytes(q.rows, q.ldb, q.Ko);
    t.unit0 = u0;
    int kc = (q.rows + h.split - 1) / h.split;
    kc = (kc + MV_GROUP_BK - 1) / MV_GROUP_BK * MV_GROUP_BK;
    t.kchunk = kc;
    u0 += mv_group_tiles(q.No, q.Ko);
  }
  *(MvGroupHeader*)table = h;
  return 0;
}

// a table the launch may trust: what mv_group_fill wrote, for this dtype and count.  Only the HOST copy can be checked; the kernels
// read the device copy, which the caller keeps byte-identical to it (include/medvill.h, mv_gemm_grouped_tn).
inline int mv_group_check_table(int dtype, int count, const void* table) {
  if (!table || count <= 0) return MV_E_ARG;
  if (dtype != MV_BF16 && dtype != MV_F16) return MV_E_DTYPE;
  const MvGroupHeader& h = *(const MvGroupHeader*)table;
  if (h.magic != MV_GROUP_MAGIC || h.count != count || count > MV_GROUP_MAX_PROBLEMS || h.n_blocks <= 0) return MV_E_ARG;
  if (h.dtype != dtype) return MV_E_DTYPE;
  const MvGroupEntry* e = (const MvGroupEntry*)((const char*)table + sizeof(MvGroupHeader));
  int u0 = 0;
  for (int i = 0; i < count; ++i) {
    const MvGroupProblemIn q = {e[i].A, e[i].B, e[i].C, e[i].lda, e[i].ldb, e[i].ldc, e[i].M, e[i].N, e[i].K};
    const int rc = mv_group_check_problem(q);
    if (rc) return rc;
    if (e[i].bytesA != mv_group_operand_bytes(e[i].K, e[i].lda, e[i].M) || e[i].bytesB != mv_group_operand_bytes(e[i].K, e[i].ldb, e[i].N)) return MV_E_ARG;
    if (e[i].unit0 != u0 || e[i].kchunk <= 0 || (e[i].kchunk % MV_GROUP_BK) != 0 || (long long)e[i].kchunk * h.split < e[i].K) return MV_E_ARG;
    u0 += mv_group_tiles(e[i].M, e[i].N);
  }
  const int rem = h.units % h.n_blocks;
  if (h.units != u0 || h.split != mv_group_tail_split(rem, h.n_blocks) || h.tail != (h.split > 1 ? rem : 0) || h.direct != h.units - h.tail) return MV_E_ARG;
  return 0;
}

inline size_t mv_group_workspace_bytes(const void* table) {
  if (!table) return 0;
  const MvGroupHeader& h = *(const MvGroupHeader*)table;
  if (h.magic != MV_GROUP_MAGIC || h.tail <= 0 || h.split <= 1) return 0;
  return (size_t)h.tail * h.split * MV_GROUP_TILE * MV_GROUP_TILE * sizeof(float);
}
#endif
