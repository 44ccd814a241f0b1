// Attention masks: packing of the [B,L,L] mask into bits + tile classes, and the dropout keep-bit generator.
#include "mv_attn.h"

// =========================================================================================
// mask packing
// =========================================================================================
__global__ void mask_pack_kernel(const int64_t* __restrict__ mask, int ndim, int B, int L, int W, uint32_t* __restrict__ bits) {
  // one wave per (b, i) row
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B * L) return;
  const int b = wave / L, i = wave - b * L;
  const int64_t* row = (ndim == 3) ? mask + ((size_t)b * L + i) * L : mask + (size_t)b * L;
  uint32_t* out = bits + ((size_t)b * L + i) * W;
  for (int j0 = 0; j0 < L; j0 += 64) {
    const int j = j0 + lane;
    const bool v = (j < L) && (row[j] != 0);
    const unsigned long long bal = __ballot(v);
    if (lane == 0) {
      out[j0 >> 5] = (uint32_t)bal;
      if ((j0 >> 5) + 1 < W) out[(j0 >> 5) + 1] = (uint32_t)(bal >> 32);
    }
  }
}

// one wave per (b, tq): class of every 64x64 tile of that query-tile row
__global__ void mask_tileinfo_kernel(const uint32_t* __restrict__ bits, int B, int L, int W, int T, uint8_t* __restrict__ info) {
  const int b = blockIdx.x / T, tq = blockIdx.x - b * T;
  const int lane = threadIdx.x;
  const int i = tq * 64 + lane;
  const bool rv = i < L;
  const uint32_t* row = bits + ((size_t)b * L + (rv ? i : 0)) * W;
  bool row_any = false;
  unsigned long long all0_m = 0, all1_m = 0;  // per-tile flags (T <= 64)
  for (int tk = 0; tk < T; ++tk) {
    const int w0 = 2 * tk;
    unsigned long long w = 0;
    if (rv) {
      w = row[w0];
      if (w0 + 1 < W) w |= ((unsigned long long)row[w0 + 1]) << 32;
    }
    const int ncol = min(64, L - tk * 64);
    const unsigned long long full = (ncol == 64) ? ~0ull : ((1ull << ncol) - 1ull);
    w &= full;
    row_any |= (w != 0);
    const bool a0 = __all(!rv || w == 0);
    const bool a1 = __all(!rv || w == full);
    if (a0) all0_m |= (1ull << tk);
    if (a1) all1_m |= (1ull << tk);
  }
  const bool rows_ok = __all(!rv || row_any);
  if (lane < T) {
    const int tk = lane;
    uint8_t c = 2;
    if ((all1_m >> tk) & 1) c = 1;
    else if (((all0_m >> tk) & 1) && rows_ok) c = 0;
    info[((size_t)b * T + tq) * T + tk] = c;
  }
}

// bits straight from per-sample descriptors {family, n2, vl}: the closed forms of SURVEY Appendix B
// (data/dataset_origin.py:138-176).  family: 0 full, 1 s2s, 2 BAR, 3 non-cross, 4 1-D (== full as a [L,L] matrix)
__global__ void mask_build_kernel(const int32_t* __restrict__ desc, int B, int L, int W, uint32_t* __restrict__ bits) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B * L) return;
  const int b = wave / L, i = wave - b * L;
  const int fam = desc[3 * b], n2 = desc[3 * b + 1], vl = desc[3 * b + 2];
  uint32_t* out = bits + ((size_t)b * L + i) * W;
  for (int j0 = 0; j0 < L; j0 += 64) {
    const int j = j0 + lane;
    bool v;
    switch (fam) {
      case 1: v = (j < n2) || (i >= n2 && j >= n2 && j <= i); break;
      case 2: v = (i < n2) || (j < n2) || (j <= i); break;
      case 3: v = (i < n2) == (j < n2); break;
      default: v = j < vl; break;
    }
    v = v && (j < L);
    const unsigned long long bal = __ballot(v);
    if (lane == 0) {
      out[j0 >> 5] = (uint32_t)bal;
      if ((j0 >> 5) + 1 < W) out[(j0 >> 5) + 1] = (uint32_t)(bal >> 32);
    }
  }
}

extern "C" int mv_mask_build(const int32_t* desc, int B, int L, uint32_t* bits, uint8_t* tileinfo, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!desc || !bits || !tileinfo || B <= 0 || L <= 0) return MV_E_ARG;
  const int W = (L + 31) / 32, T = (L + 63) / 64;
  if (T > 64) return MV_E_SHAPE;
  const long long waves = (long long)B * L;
  hipLaunchKernelGGL(mask_build_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, desc, B, L, W, bits);
  MV_CHECK_LAUNCH();
  hipLaunchKernelGGL(mask_tileinfo_kernel, dim3(B * T), dim3(64), 0, stream, bits, B, L, W, T, tileinfo);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_mask_pack(const int64_t* mask, int mask_ndim, int B, int L, uint32_t* bits, uint8_t* tileinfo, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!mask || !bits || !tileinfo || B <= 0 || L <= 0) return MV_E_ARG;
  if (mask_ndim != 2 && mask_ndim != 3) return MV_E_SHAPE;   // NotImplementedError in cxrbert_origin.py:80-81
  const int W = (L + 31) / 32, T = (L + 63) / 64;
  if (T > 64) return MV_E_SHAPE;
  const long long waves = (long long)B * L;
  hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, mask, mask_ndim, B, L, W, bits);
  MV_CHECK_LAUNCH();
  hipLaunchKernelGGL(mask_tileinfo_kernel, dim3(B * T), dim3(64), 0, stream, bits, B, L, W, T, tileinfo);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

// One thread per 64-bit word.  The word's 64 keep decisions are 64 independent PL-bit uniforms compared with the threshold
// thr = round(p * 2^PL), evaluated bit-sliced: PL bit-planes of 64 random bits each (two 32-bit hashes of a counter), most
// significant plane first -- lt collects the lanes already known to be below the threshold, eq those still equal to its prefix.
// drop = (x < thr), so P(drop) = thr / 2^PL.  No cross-lane work; the kernel is bound by the hashes' quarter-rate multiplies
// (profiles/r03_notes.txt: 2 * PL hashes per word, time proportional to PL -- until round 5 cut the planes after the eighth, see below).
template <int PL>
__global__ __launch_bounds__(256) void attn_dropmask_kernel(unsigned k0, unsigned k1, unsigned thr16, int A, int L, int NQB, int NKT,
                                                            const int32_t* __restrict__ cu, unsigned long long* __restrict__ out, size_t nwords) {
  // thread blocks of one (sample, head) are spread over the dispatch order (see att_block: its later query blocks are the empty ones)
  const unsigned nbh = (unsigned)(nwords / ((size_t)NQB * NKT * 32)), per = gridDim.x / nbh;
  const unsigned lb = (per * nbh == gridDim.x) ? (blockIdx.x % nbh) * per + blockIdx.x / nbh : blockIdx.x;
  const size_t w = (size_t)lb * 256 + threadIdx.x;
  if (w >= nwords) return;
  const size_t blk = w >> 5;
  const int kt = (int)(blk % NKT), qb = (int)((blk / NKT) % NQB);
  const int b = (int)(blk / ((size_t)NKT * NQB * A));
  const int Lv = cu ? cu[b + 1] - cu[b] : L;
  if (qb * 32 >= Lv || kt * 64 >= Lv) return;        // no kernel ever looks at a block without an existing query or key
  const unsigned base = (unsigned)w * 32u;
  unsigned long long lt = 0ull, eq = ~0ull;
  // PL > 8: only the 8 most significant planes are evaluated bit-sliced.  After them a lane is still undecided with probability 2^-8
  // (its high byte equals the threshold's): 0.25 lanes per word on average, and those few draw their remaining PL - 8 bits one lane at a
  // time from single extra hashes (counters below the planes').  Same distribution -- P(drop) = thr / 2^PL exactly -- for 16 + ~2 hashes
  // per word instead of 2 * PL (round 5: 36 -> 23 us per layer at PL = 16).
  constexpr int SL = PL > 8 ? PL - 8 : 0;          // planes left to the serial tail
#pragma unroll
  for (int j = PL - 1; j >= SL; --j) {
    const unsigned long long x = ((unsigned long long)mv_hash32(base + 2 * j, k0, k1) << 32) | mv_hash32(base + 2 * j + 1, k0, k1);
    const unsigned long long tb = 0ull - (unsigned long long)((thr16 >> j) & 1u);      // all ones where the threshold has this bit
    lt |= eq & ~x & tb;
    eq &= x ^ ~tb;
  }
  if constexpr (SL > 0) {
    const unsigned lo = thr16 & ((1u << SL) - 1u);
    constexpr int PER = 32 / SL;                    // lanes served by one hash
    unsigned r = 0, ctr = 0;
    int have = 0;
    while (eq) {
      const int l = __builtin_ctzll(eq);
      eq &= eq - 1ull;
      if (have == 0) { r = mv_hash32(base + ctr, k0, k1); ++ctr; have = PER; }
      const unsigned x = r & ((1u << SL) - 1u);
      r >>= SL;
      --have;
      if (x < lo) lt |= 1ull << l;
    }
  }
  out[w] = ~lt;
}

extern "C" int mv_attn_dropmask(float p_drop, unsigned long long drop_key, int B, int L, int A, const int32_t* cu, uint32_t* dropbits,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dropbits || B <= 0 || L <= 0 || A <= 0 || p_drop <= 0.f || p_drop >= 1.f) return MV_E_ARG;
  const size_t nwords = dropbits_words(B, L, A) / 2;         // 64-bit words
  if (nwords * 32 >= (1ull << 32)) return MV_E_SHAPE;         // 32 hash counters per word, 32-bit counters
  const int rc = dropbits_check(p_drop, dropbits, B, L, A);
  if (rc) return rc;
#define DM_LAUNCH(PL_)                                                                                                                  \
  hipLaunchKernelGGL(attn_dropmask_kernel<PL_>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, stream, (unsigned)(drop_key & 0xffffffffULL), \
                     (unsigned)(drop_key >> 32), attn_thr16(p_drop), A, L, (L + 31) / 32, (L + 63) / 64, cu, (unsigned long long*)dropbits, nwords)
  if (g_mv_attn_planes == 8) DM_LAUNCH(8);
  else if (g_mv_attn_planes == 12) DM_LAUNCH(12);
  else DM_LAUNCH(16);
#undef DM_LAUNCH
  MV_CHECK_LAUNCH();
  return MV_OK;
}
