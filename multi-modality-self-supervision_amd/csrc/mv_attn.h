// What the attention translation units share (mv_attn.hip: file map and overview).
#pragma once
#include "mv_dispatch.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
// Timing experiments on the forward kernel were compile-time switches here until the kernels were split into units (-DATT_ABL=<bits>: no
// per-tile barrier, no exponentials, dropout masks from constants instead of scalar loads, no cross-half maximum, no P.V products, no Q.K
// products, no LDS-DMA, grid dispatch alone, prologue only, prologue + epilogue; results WRONG by construction).  Single ablations moved the
// forward by 4-8 % each -- no one resource is the bound -- and the prologue + epilogue figures led to store_rows_tile: profiles/r04_notes.txt.
// What is left is the one tool that is run again:
// ATT_PROF = 1: phase profile -- every wave reads the shader clock at the phase boundaries of its tile loop, thread 0 of each block adds the
// phase totals to g_att_prof[kernel][phase] (0 prologue, 1 wait for the tile's LDS-DMA, 2 barrier, 3 tile body, 4 issue of the next tile,
// 5 epilogue, 7 = number of blocks); mv_debug_attn_prof() returns and clears them (profiles/tools/attn_phase.py builds the variant library
// from mv_attn_mfma.hip, which holds the counters).  0 in the product build.
#ifndef ATT_PROF
#define ATT_PROF 0
#endif
#if ATT_PROF
#define PROF_DECL unsigned long long pt_ = clock64(), pacc_[6] = {0, 0, 0, 0, 0, 0}; unsigned long long ptile_[6] = {0, 0, 0, 0, 0, 0}
#define PROF_TILE_ARGS , unsigned long long (&ptile_)[6]
#define PROF_TILE_PASS , ptile_
#define PROF_T0 unsigned long long tt_ = clock64()
#define PROF_T(i, dep) do { asm volatile("s_nop 0" ::"v"(dep)); const unsigned long long n_ = clock64(); ptile_[i] += n_ - tt_; tt_ = n_; } while (0)
#define PROF_MARK(i) do { const unsigned long long n_ = clock64(); pacc_[i] += n_ - pt_; pt_ = n_; } while (0)
#define PROF_FLUSH(k) do { if (threadIdx.x == 0) { for (int i_ = 0; i_ < 6; ++i_) { atomicAdd(&g_att_prof[k][i_], pacc_[i_]); atomicAdd(&g_att_tile[k][i_], ptile_[i_]); } atomicAdd(&g_att_prof[k][7], 1ull); } } while (0)
#else
#define PROF_DECL
#define PROF_MARK(i)
#define PROF_FLUSH(k)
#define PROF_TILE_ARGS
#define PROF_TILE_PASS
#define PROF_T0
#define PROF_T(i, dep)
#endif
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f
#define MASK_ADD (-10000.0f)

struct AttnArgs {
  const bf16_t* qkv; const bf16_t* ctx; const bf16_t* dctx; bf16_t* out; bf16_t* dqkv;
  bf16_t* out2;   // forward, f16 operands only (nullable): bf16 copy of the context for the backward's gradient products
  const uint32_t* bits; const uint8_t* info; float* lse; const float* lse_in; const float* delta; float* delta_out;
  int B, L, A, H, W, T;
  float scale;
  unsigned bytes_qkv, bytes_ctx;
  unsigned bytes_stat, bytes_bits;     // sizes of lse / delta ([B,A,L] f32) and of the mask words, for the LDS-DMA descriptors
  // attention-probability dropout (drop_on): the mask is a tensor of precomputed keep-bits (mv_attn_dropmask): per (b*A + h,
  // 32-query block, 64-key tile) 32 x u64, word 16*kk + r, bit l = keep(query 32*qb + (l & 31), key 64*kt + 32*kk + acc_row(r, l >> 5))
  // -- i.e. the 64-lane select mask of accumulator register r of the forward / dQ kernels (queries on the lanes), and for the
  // dK/dV kernel (keys on the lanes) one dword per key holding the bits of 32 queries.  No kernel hashes: one select per score
  // element (the kernels are bound by vector-instruction issue).  Survivors are scaled by inv_keep.
  int drop_on;
  float inv_keep;
  const uint32_t* dropbits;
  unsigned bytes_dbits;
  int NQB, NKT;     // 32-query blocks / 64-key tiles per (b, h) in dropbits
  // packed rows (nullable): sample b owns rows cu[b] .. cu[b+1]-1 of qkv / ctx / dctx / out / dqkv, i.e. only its first
  // cu[b+1]-cu[b] positions exist; mask words, lse, delta and the dropout counter keep their logical [B, L] indexing
  const int32_t* cu;
  // query limit (nullable): only the first qlim[b] rows of sample b are QUERIES (every row is a key).  The forward leaves the context /
  // lse of the other rows untouched, the backward writes zero dQ rows for them and ignores their dctx rows.  Used for the last encoder
  // layer, whose rows are reordered so that the rows the heads consume come first (mv_tail_perm).
  const int32_t* qlim;
  int order;        // att_block(): block -> (row block, head, sample) order
};
// ---- precomputed dropout keep-bits -------------------------------------------------------------------------------------------
typedef unsigned long long u64x8 __attribute__((ext_vector_type(8)));
// 16 select masks (one 32-key half of a tile) from a wave-uniform address.  The pointer is made provably uniform (readfirstlane) and
// read through the constant address space, so hipcc emits two s_load_dwordx16 that IT tracks: it may issue them ahead of the tile's
// last MFMAs and waits where the first select needs them (round 3 first had both loads and their wait inside one asm statement, i.e.
// a full scalar-memory round trip in front of every 32-key half: forward -2..5 %, backward unchanged).
__device__ __forceinline__ void sload_masks16(const void* p, u64x8& m0, u64x8& m1) {
  const unsigned long long v = (unsigned long long)(uintptr_t)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  typedef const u64x8 __attribute__((address_space(4))) cmask_t;
  cmask_t* q = (cmask_t*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  m0 = q[0];
  m1 = q[1];
}
// Selects by a 64-lane mask held in an SGPR pair: one VALU instruction (v_cndmask_b32 with an SGPR condition).  hipcc pads no hazard
// for an asm statement, so the VGPR inputs must never be the direct result of an MFMA (18 wait states) or of a transcendental
// (1 wait state): sel_set_else() is fed with fma results, sel_lane_after() names a second value `after` that a compiler-scheduled
// VALU instruction computed FROM x, which orders the statement behind that instruction.
__device__ __forceinline__ float sel_set_else(float if_set, float if_clear, unsigned long long m) {
  float o;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(o) : "v"(if_clear), "v"(if_set), "s"(m));
  return o;
}
__device__ __forceinline__ float sel_lane_after(float x, float after, unsigned long long m) {
  float o;
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(o) : "v"(x), "s"(m), "v"(after));
  return o;
}
// one bit of the keep-bits for any (query, key): the plain VALU kernels' view of the same tensor
__device__ __forceinline__ bool attn_keep_bit(const unsigned long long* db, int NQB, int NKT, size_t bh, int q, int k) {
  const int k32 = k & 31, r = ((k32 >> 3) << 2) | (k32 & 3), hf = (k32 >> 2) & 1;
  const unsigned long long w = db[((bh * (size_t)NQB + (q >> 5)) * (size_t)NKT + (k >> 6)) * 32 + ((k >> 5) & 1) * 16 + r];
  return (w >> ((q & 31) + 32 * hf)) & 1ull;
}
__device__ __forceinline__ float and_bits(float x, int t) { return __uint_as_float(__float_as_uint(x) & (unsigned)t); }
__device__ __forceinline__ size_t dbits_block(const AttnArgs& a, size_t bh, int qb, int kt) {      // first u64 of a (32 x 64) block
  return ((bh * (size_t)a.NQB + qb) * (size_t)a.NKT + kt) * 32;
}

// dual-use LDS image of a [64 rows][64 x bf16] tile: 128-B rows, 16-B chunk index XORed with f(row)
__device__ __forceinline__ int att_f(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int att_off(int r, int ch) { return r * 128 + ((ch ^ att_f(r)) << 4); }

// rows of a 32x32 accumulator: element `reg` of lane-half h is row (reg&3) + 8*(reg>>2) + 4*h
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// The same tile, HBM -> LDS directly (LDS-DMA, `buffer_load ... lds`, 16 B per lane): 8 pieces of 1 KiB = 8 rows each; wave
// `wid` of NW issues pieces wid, wid + NW, ...  The LDS image of a piece is lane-linear, so the chunk swizzle of att_off() is
// applied to the per-lane SOURCE address; rows past `nrows` are zero-filled (out-of-range buffer offset).  No registers hold
// the tile, so a ring of several stages can be in flight: the kernels below keep NS - 1 tiles ahead of the one they compute on
// and retire them with counted `s_waitcnt vmcnt(N)` + one raw s_barrier per tile.
// The LDS-DMA itself is issued from inline assembly.  Through the builtin the compiler tracks the transfer as a pending LDS
// write and, having no alias information for `ds_read_b64_tr_b16`, puts `s_waitcnt vmcnt(0)` in front of the first transposed
// fragment read of every tile -- the whole ring drained once per tile, so only the transfer issued last was ever ahead.  The
// kernels below order the ring themselves (counted vmcnt + s_barrier before a stage is read, see att_wait_stage).
// (dma_rsrc_t, dma_rsrc, lds_dma16, lds_dma4: mv_common.h)
template <int NW>
__device__ __forceinline__ void tile_dma(dma_rsrc_t rs, unsigned bytes, size_t rowbase, int row0, int nrows, int ld,
                                         int col0, char* tile, int wid, int lane) {
#pragma unroll
  for (int i = 0; i < 8 / NW; ++i) {
    const int pc = wid + NW * i;
    const int r = pc * 8 + (lane >> 3), ch = (lane & 7) ^ att_f(r);
    const bool ok = (row0 + r) < nrows;
    const unsigned off = (unsigned)(((rowbase + row0 + r) * (size_t)ld + col0 + ch * 8) * 2);
    lds_dma16(rs, (MV_LDS void*)(tile + pc * 1024), ok ? off : bytes);
  }
}
template <int N> __device__ __forceinline__ void att_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// wait until at most `younger` stages (of PPW LDS-DMA instructions per wave each) are still in flight
template <int PPW>
__device__ __forceinline__ void att_wait_stage(int younger) {
  if (younger <= 0) att_wait_vmcnt<0>();
  else if (younger == 1) att_wait_vmcnt<PPW>();
  else if (younger == 2) att_wait_vmcnt<2 * PPW>();
  else att_wait_vmcnt<3 * PPW>();
}

// The two fragment reads of a tile, written out with att_off() (the functions frag_row / frag_tr, which had no caller left, were these):
//   frag_row(tile, base, s):   row-read fragment  X[idx = base + (lane&31)][k = 16*s + 8*h + j]  =  16 bytes at tile + att_off(base + l31, 2*s + h)
//   frag_tr (tile, cbase, rb): transposed fragment  A[row = cbase + (lane&31)][k = tile row rb + 8*(j>>2) + 4*h' + (j&3)]  =  two ds_read_b64_tr_b16,
//                              lo at tile + att_off(r, col >> 3) + 8 (li & 1), hi at att_off(r + 8, ..), with li = lane & 15, g = lane >> 4, h' = g >> 1,
//                              col = cbase + 16 (g & 1) + 4 (li & 3), r = rb + 4h' + (li >> 2)
// frag_row_x / frag_tr_x are the same reads with the lane-dependent part of att_off() taken out of the tile loop.  Per lane and tile-invariant:
//   rk = (lane&31)*128 + ((h ^ f0) << 4) + ((f >> 1) << 5)        f = att_f(lane & 31): bits 5-6 of rk ARE the chunk swizzle of s = 0
//   tr = (4h' + q)*128 + ((q >> 1) << 6) + ((g & 1) << 5) + ((c0 ^ h') << 4) + 8 (li & 1)
// so that, for a tile at LDS byte address T (a multiple of 128 B -- the XORs touch bits 4-6 only, and T + rk / T + tr carry nothing into them),
//   frag_row(T, base, s)      = ((T + rk) ^ (s << 5)) + 128 base                                 base = 0 / 32
//   frag_tr (T, 32 dt, rb) lo = ((T + tr) ^ (dt << 6)) + 128 rb,   hi = (... ^ 32) + 128 rb + 1024
// i.e. one add per tile and one XOR per (s) / (dt, half); everything else is an instruction immediate.  Before, hipcc rebuilt every
// address from the (per tile opaque, see dkv_tile) lane index: ~6 VALU instructions per ds_read, a quarter of the forward's issue slots.
struct FragLane { unsigned rk, tr; };
__device__ __forceinline__ FragLane frag_lane(int lane) {
  const int l31 = lane & 31, h = lane >> 5, f = att_f(l31);
  const int li = lane & 15, g = lane >> 4, hh = g >> 1, q = li >> 2, c0 = (li & 3) >> 1;
  FragLane o;
  o.rk = (unsigned)(l31 * 128 + (((h ^ f) & 1) << 4) + ((f >> 1) << 5));
  o.tr = (unsigned)((4 * hh + q) * 128 + ((q >> 1) << 6) + ((g & 1) << 5) + ((c0 ^ hh) << 4) + (li & 1) * 8);
  return o;
}
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)(MV_LDS const char*)p; }
// tk = lds_addr(tile) + FragLane::rk
__device__ __forceinline__ bf16x8 frag_row_x(unsigned tk, int base, int s) {
  return *(MV_LDS const bf16x8*)(uintptr_t)((tk ^ (unsigned)(s << 5)) + 128u * base);
}
// tt = lds_addr(tile) + FragLane::tr
__device__ __forceinline__ bf16x8 frag_tr_x(unsigned tt, int dt, int rb) {
  const unsigned t = tt ^ (unsigned)(dt << 6);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((MV_LDS bf16x4*)(uintptr_t)(t + 128u * rb));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((MV_LDS bf16x4*)(uintptr_t)((t ^ 32u) + 128u * rb + 1024u));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 pack8(const f32x16& v, int s2) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16_t)v[8 * s2 + j];
  return r;
}
// 32x32x16 MFMA / accumulator packing in the operand encoding of the kernel: F16 = f16 bit patterns carried in bf16x8
template <bool F16>
__device__ __forceinline__ f32x16 mma32(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ bf16x8 pack8t(const f32x16& v, int s2) {
  if constexpr (F16) {
    f16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (f16_t)v[8 * s2 + j];
    return __builtin_bit_cast(bf16x8, r);
  } else {
    return pack8(v, s2);
  }
}
template <bool F16>
__device__ __forceinline__ float frag_elem(bf16x8 v, int j) {
  if constexpr (F16) return (float)__builtin_bit_cast(f16x8, v)[j];
  else return (float)v[j];
}
template <bool F16>
__device__ __forceinline__ void store4_16(bf16_t* p, float a, float b, float c, float d) {
  const f32x4 v = {a, b, c, d};
  if constexpr (F16) st4<f16_t>((f16_t*)p, v);
  else st4<bf16_t>(p, v);
}
__device__ __forceinline__ bf16x8 load_rowfrag_global(__amdgpu_buffer_rsrc_t rs, unsigned bytes, size_t row, bool ok, int ld,
                                                      int col) {
  const unsigned off = (unsigned)((row * (size_t)ld + col) * 2);
  u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off : bytes, 0, 0);
  return __builtin_bit_cast(bf16x8, v);
}

// tile classes of the block's two 64-row tiles, fetched ONCE (lane t holds tile t) and turned into wave-uniform bit
// masks: the K loop then walks set bits instead of issuing dependent global loads per tile
// (The class of tile t for a wave -- !wave_on ? 0 : bit t of w_is1 ? 1 : bit t of w_nz ? 2 : 0 -- and the ring bookkeeping over `need` stay
// spelled out in the three kernels: as helpers they change the kernels' code)
struct TileMasks { unsigned long long need, w_nz, w_is1; };
// The block owns tiles ta and ta + 1 of one axis of the sample's [T query tiles][T key tiles] class matrix and walks the other axis.
// BY_KEY = false: it owns query tiles (forward, dQ), lane t holds key tile t; true: it owns key tiles (dK/dV), lane t holds query tile t.
// t_wave: the wave's own tile.  (The two index expressions stay spelled out under a template argument: behind a helper, a run-time flag or
// two strides the same loads cost the forward and the dQ kernel seven instructions -- DESIGN.md 8v.)
template <bool BY_KEY>
__device__ __forceinline__ TileMasks load_tile_masks(const uint8_t* info, int b, int T, int ta, int t_wave, int lane) {
  uint8_t c0 = 0, c1 = 0;
  if (lane < T) {
    if constexpr (BY_KEY) {
      c0 = info[((size_t)b * T + lane) * T + ta];
      if (ta + 1 < T) c1 = info[((size_t)b * T + lane) * T + ta + 1];
    } else {
      c0 = info[((size_t)b * T + ta) * T + lane];
      if (ta + 1 < T) c1 = info[((size_t)b * T + ta + 1) * T + lane];
    }
  }
  const uint8_t cw = (t_wave == ta) ? c0 : c1;
  TileMasks m;
  m.need = __ballot(c0 != 0 || c1 != 0);
  m.w_nz = __ballot(cw != 0);
  m.w_is1 = __ballot(cw == 1);
  return m;
}
// Row plan of sample b: its first row_count() positions exist as rows (packed rows, AttnArgs::cu), the first query_count() of those are
// queries (AttnArgs::qlim), and row_base() is its first row in qkv / ctx / dctx / out / dqkv.  Mask words, lse and delta keep their logical
// [B, L] indexing.  Three functions, not one that returns all three: each kernel asks where it needs the value, between its early exits
// (together, ahead of them, they cost the forward 21 instructions, dQ 17 and dK/dV 4 -- DESIGN.md 8v).
__device__ __forceinline__ int row_count(const AttnArgs& a, int b) { return a.cu ? a.cu[b + 1] - a.cu[b] : a.L; }
__device__ __forceinline__ int query_count(const AttnArgs& a, int b, int Lv) { return a.qlim ? min(Lv, a.qlim[b]) : Lv; }
__device__ __forceinline__ size_t row_base(const AttnArgs& a, int b) { return a.cu ? (size_t)a.cu[b] : (size_t)b * a.L; }
__device__ __forceinline__ int next_tile(unsigned long long need, int after, int n) {   // first set bit > after, else n
  const unsigned long long rem = (after >= 63) ? 0ull : (need >> (after + 1));
  return rem ? after + 1 + (int)__builtin_ctzll(rem) : n;
}

// Block -> (128-row block xb, head, sample).  Workgroups go to the 8 XCDs round-robin in dispatch order (x fastest), each XCD has its own
// 4 MiB L2, and the row blocks of one (sample, head) pair all stream the SAME K / V rows (forward, dQ) or Q / dO rows (dK/dV): 128 KiB at
// L = 512.  Three orders have existed:
//   blockIdx as is (rounds 1-2): the row block is the fastest index, so the pair's four row blocks go to four DIFFERENT XCDs -- and XCD k
//     only ever sees row block k % 4, nearly empty for the last block of a packed sample: two XCDs idled.
//   order 0 (rounds 3-5, the default): the row block is the SLOWEST index.  Even load; the row blocks of a pair run a whole wave of ~768
//     resident blocks apart, so every block fetches its K / V over the fabric (profiles/r04_attn_pmc.json: 2.97x the algorithmic
//     bytes, L2 hit 16-28 %) -- which is NOT what bounds these kernels:
//   order 1 (round 5 experiment, debug knob attn_order): flat = 8 * (group * nxb + xb) + x, pair = 8 * group + x.  The nxb row blocks of
//     a pair are 8 apart in dispatch order -- consecutive blocks of ONE XCD, resident together -- so the pair's K / V is fetched into
//     that L2 once.  Measured in one process against order 0 (profiles/tools/attn_order_ab.py, profiles/r05_notes.txt): bidirectional
//     packed forward 82.5 -> 81.2 us, backward 257 -> 266 us; BAR forward 97 -> 116, backward 293 -> 353; seq2seq backward 190 -> 246; whole
//     step 24.22 -> 24.36 ms.  With row-dependent masks the blocks resident together then differ in length by up to 4x and the launch
//     ends on a tail of long blocks; with uniform masks nothing is gained either: the kernels wait on dependent latency inside a tile
//     (DESIGN.md 8), not on fabric bandwidth.  Pairs beyond the last multiple of 8 fall back to the row-block-fastest walk.
//   Placement is a speed matter only: nothing depends on it for correctness (outputs are bit-identical in both orders).
__device__ __forceinline__ void att_block_at(int order, int& xb, int& head, int& b) {
  const int flat = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int nxb = gridDim.x, nhb = gridDim.y * gridDim.z;
  int pair;
  if (order == 0) {
    xb = flat / nhb;
    pair = flat - xb * nhb;
  } else {
    const int full = (nhb >> 3) << 3;               // pairs covered by whole groups of 8
    if (flat < full * nxb) {
      const int x = flat & 7, k = flat >> 3;
      const int g = k / nxb;
      xb = k - g * nxb;
      pair = 8 * g + x;
    } else {
      const int r = flat - full * nxb;
      pair = full + r / nxb;
      xb = r - (pair - full) * nxb;
    }
  }
  b = pair / gridDim.y;
  head = pair - b * gridDim.y;
}
__device__ __forceinline__ void att_block(const AttnArgs& a, int& xb, int& head, int& b) { att_block_at(a.order, xb, head, b); }
// A wave's [32 rows][64 columns] 16-bit output tile leaves as WHOLE 128-byte row segments.  The tile sits in two 32x32 accumulators with
// the rows on the lanes (lane (l31, h), register reg of acc[dt]: row l31, column 32 dt + acc_row(reg, h)), so a direct store writes 8 bytes of
// 32 different rows per instruction and every 128-byte line of the output is written in eight pieces by eight instructions: measured on
// the forward (profiles/r04_notes.txt) the epilogue alone cost 25 of the kernel's 100 us.  Here the tile goes through a private
// 32 x 144-byte LDS patch (ds_write_b64 per 4 columns, ds_read_b128 per 8): 16 bytes per lane, 8 full rows per store instruction.
// `rows_ok`: rows [0, rows_ok) of the tile exist in the output; `patch` is this wave's own 4608-byte region (callers barrier first).
#define ATT_PATCH_BYTES 4608
template <bool F16>
__device__ __forceinline__ void store_rows_tile(char* patch, const f32x16 (&acc)[2], float scale, bool lane_ok, bf16_t* g_row0, size_t ld,
                                                int rows_ok, int lane) {
  const int l31 = lane & 31, h = lane >> 5;
  // The patch is written and read by ONE wave (different lanes touch the same bytes).  The hardware completes a wave's LDS operations in
  // order; the COMPILER is told so explicitly -- a wavefront-scope fence pair around a wave barrier (no instruction: a scheduling and
  // memory-ordering point) before the writes (a previous use of the same patch: dK then dV) and between the writes and the reads --
  // instead of relying on it failing to prove the addresses disjoint.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v = {acc[dt][4 * g] * scale, acc[dt][4 * g + 1] * scale, acc[dt][4 * g + 2] * scale, acc[dt][4 * g + 3] * scale};
      if (!lane_ok) v = (f32x4){0.f, 0.f, 0.f, 0.f};        // (a select, not a product: the lane's accumulators may hold anything)
      bf16_t* dst = (bf16_t*)(patch + l31 * 144) + 32 * dt + 8 * g + 4 * h;
      if constexpr (F16) st4<f16_t>((f16_t*)dst, v);
      else st4<bf16_t>(dst, v);
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (lane >> 3) + 8 * i, c = lane & 7;
    const u32x4 v = *(const u32x4*)(patch + r * 144 + 16 * c);
    if (r < rows_ok) *(u32x4*)(g_row0 + (size_t)r * ld + 8 * c) = v;
  }
}

// ---- host ----
static inline size_t dropbits_words(int B, int L, int A) { return (size_t)B * A * ((L + 31) / 32) * ((L + 63) / 64) * 64; }   // uint32 count
// bits per uniform of mv_attn_dropmask (8, 12 or 16): P(drop) = thr / 2^planes with thr = round(p * 2^planes); survivors are scaled
// by 2^planes / (2^planes - thr).  p = 0.1: 16 -> 0.100006, 12 -> 0.100098, 8 -> 0.101563.
#define g_mv_attn_planes (mv_knob(MV_KNOB_ATTN_PLANES))
static inline unsigned attn_thr16(float p) {          // threshold at the current plane count
  const int full = 1 << g_mv_attn_planes;
  int t = (int)(p * (float)full + 0.5f);
  return (unsigned)(t < 1 ? 1 : (t > full - 1 ? full - 1 : t));
}
static inline float attn_inv_keep(float p) {
  const float full = (float)(1 << g_mv_attn_planes);
  return p > 0.f ? full / (full - (float)attn_thr16(p)) : 1.0f;
}
// p_drop > 0 needs the keep-bits (64-byte aligned: scalar loads of 64-byte pieces; 32-bit buffer offsets)
static inline int dropbits_check(float p_drop, const uint32_t* dropbits, int B, int L, int A) {
  if (p_drop <= 0.f) return MV_OK;
  if (p_drop >= 1.f || !dropbits) return MV_E_ARG;
  if ((((uintptr_t)dropbits) & 63) || dropbits_words(B, L, A) * 4 >= 0x7fffffffULL) return MV_E_SHAPE;
  return MV_OK;
}
// the fields that AttnArgs, SArgs, ProbArgs and PSArgs have in common: sizes, scale, keep-bits (null = dropout off) and their geometry
template <typename Args>
static inline void attn_fill_common(Args& a, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits) {
  a.B = B; a.L = L; a.A = A; a.H = A * dh; a.W = (L + 31) / 32;
  a.scale = 1.0f / sqrtf((float)dh);
  a.dropbits = p_drop > 0.f ? (decltype(a.dropbits))dropbits : nullptr; a.inv_keep = attn_inv_keep(p_drop);
  a.NQB = (L + 31) / 32; a.NKT = (L + 63) / 64;
}

// launchers across the units (C++ names, hidden like mv_knob): the entry points validate and choose, these fill their kernels' arguments
// and launch; each returns the int status of its last launch
#define MV_ATTN_HIDDEN __attribute__((visibility("hidden")))
MV_ATTN_HIDDEN int mv_attn_launch_fwd(const AttnArgs& a, bool f16, hipStream_t stream);      // mv_attn_mfma.hip
MV_ATTN_HIDDEN int mv_attn_launch_bwd(const AttnArgs& a, bool f16, hipStream_t stream);      // dQ (publishes delta), then dK/dV
MV_ATTN_HIDDEN int mv_attn_simple_fwd(int dtype, const void* qkv, const uint32_t* bits, void* ctx, float* lse, int B, int L, int A, int dh, float p_drop,
                                      const uint32_t* dropbits, hipStream_t stream);           // mv_attn_simple.hip
MV_ATTN_HIDDEN int mv_attn_simple_bwd(int dtype, const void* qkv, const void* ctx, const void* dctx, const float* lse, const uint32_t* bits, void* dqkv,
                                      float* delta, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits, hipStream_t stream);
