// Attention probabilities (mv_attn_probs): the MFMA kernel, its VALU form and the entry point.
#include "mv_attn.h"

// =========================================================================================
// attention probabilities (mv_attn_probs)
// =========================================================================================
// P[b,a,i,j] = exp(q_i.k_j / sqrt(dh) + (mask ? 0 : -10000) - lse[b,a,i]) from a layer's qkv and the forward's lse: the matrix the
// flash-style forward never stores, written out for callers that want attention maps.  With dropout it is the matrix the context was
// computed from (keep-bits of mv_attn_dropmask, survivors times inv_keep); with head_mean the arithmetic mean over the heads.  The kernel
// is bound by the bytes it writes (B.A.L.L elements against B.L.3H read).
struct ProbArgs {
  const bf16_t* qkv; const uint32_t* bits; const uint8_t* info; const float* lse; void* out;
  int B, L, A, H, W, T;
  float scale;
  unsigned bytes_qkv;
  int drop_on;
  float inv_keep;
  const uint32_t* dropbits;
  int NQB, NKT;
  int head_mean;    // 1: out is [B, L, L], the mean over the A heads, accumulated in f32 by the one block that owns the tile
  int vec;          // 1: every output row starts on a 16-byte boundary (L a multiple of 16 / sizeof(out element)): 16-byte stores
  int order;        // att_block_at()
};

// A wave's [32 queries][64 keys] probabilities sit in two 32x32 accumulators with the QUERY on the lane (S^T = K.Q^T, as in the forward): lane
// (l31, h) holds, for query l31, keys 32 kk + acc_row(reg, h) -- four consecutive keys per register quadruple.  They leave through the wave's own
// 32 x 144-byte LDS patch (the forward epilogue's, store_rows_tile) so that every store instruction writes whole rows: 16 bytes per lane and
// 8 rows x 128 bytes per instruction on the aligned route; one element per lane and whole 128-byte row segments on the route for lengths whose
// rows do not start on 16-byte boundaries.  f32 output takes the patch twice (32 keys x 4 bytes = 128 bytes per row and pass).
// Rows [0, rows_ok) and columns [0, cols_ok) of the tile exist in the output: nothing else is written.
__device__ __forceinline__ void probs_patch_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <typename TO>
__device__ __forceinline__ void probs_store_tile(char* patch, const f32x16 (&acc)[2], TO* g_row0, size_t ldo, int rows_ok, int cols_ok, bool vec,
                                                 int lane) {
  const int l31 = lane & 31, h = lane >> 5;
  if constexpr (sizeof(TO) == 4) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      probs_patch_sync();
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = {acc[kk][4 * g], acc[kk][4 * g + 1], acc[kk][4 * g + 2], acc[kk][4 * g + 3]};
        *(f32x4*)(patch + l31 * 144 + (8 * g + 4 * h) * 4) = v;
      }
      probs_patch_sync();
      if (vec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = (lane >> 3) + 8 * i, c = 32 * kk + 4 * (lane & 7);
          const u32x4 v = *(const u32x4*)(patch + r * 144 + 16 * (lane & 7));
          if (r < rows_ok && c < cols_ok) *(u32x4*)(g_row0 + (size_t)r * ldo + c) = v;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int r = 2 * i + h, c = 32 * kk + l31;
          const float v = *(const float*)(patch + r * 144 + 4 * l31);
          if (r < rows_ok && c < cols_ok) g_row0[(size_t)r * ldo + c] = v;
        }
      }
    }
  } else {
    probs_patch_sync();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = {acc[kk][4 * g], acc[kk][4 * g + 1], acc[kk][4 * g + 2], acc[kk][4 * g + 3]};
        st4<TO>((TO*)(patch + l31 * 144) + 32 * kk + 8 * g + 4 * h, v);
      }
    probs_patch_sync();
    if (vec) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = (lane >> 3) + 8 * i, c = 8 * (lane & 7);
        const u32x4 v = *(const u32x4*)(patch + r * 144 + 16 * (lane & 7));
        if (r < rows_ok && c < cols_ok) *(u32x4*)(g_row0 + (size_t)r * ldo + c) = v;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        const TO v = *(const TO*)(patch + r * 144 + 2 * lane);
        if (r < rows_ok && lane < cols_ok) g_row0[(size_t)r * ldo + lane] = v;
      }
    }
  }
}

// the probabilities of one (head, 64-key tile) for a wave's 32 queries, in place of the scores.  MASKED: the tile reads its mask words (class 2);
// class 1 tiles read none.  Keys past L get whatever the zero-filled rows give: they are never stored.
template <bool MASKED>
__device__ __forceinline__ void probs_tile(const ProbArgs& a, f32x16 (&st)[2], const uint32_t* myw, bool q_ok, int k0, float c2, float lse2, int h,
                                           int lane, const unsigned long long* mp) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    uint32_t w = 0xffffffffu;
    if (MASKED) { const int wi = (k0 >> 5) + kk; w = (q_ok && wi < a.W) ? myw[wi] : 0xffffffffu; }
    u64x8 m0, m1;
    if (a.drop_on) sload_masks16(mp + 16 * kk, m0, m1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = acc_row(r, h);
      const float v = fmaf(st[kk][r], c2, (MASKED && !((w >> kr) & 1u)) ? MASK_ADD * LOG2E : 0.f);
      float pv = fexp2(v - lse2);
      if (a.drop_on) {
        const unsigned long long m = r < 8 ? m0[r & 7] : m1[r & 7];
        pv = ((m >> lane) & 1ull) ? pv * a.inv_keep : 0.f;
      }
      st[kk][r] = pv;
    }
  }
}

// One block per (sample, head -- or all heads when head_mean --, 64-query tile); block -> (tile, head, sample) through att_block_at(), so the
// query tile is not the fastest dispatch index.  Wave w owns the tile's queries 32 (w & 1) .. +31 and the key tiles of parity w >> 1: per
// key tile four K fragments straight from global memory (row-read layout, 16 bytes per lane), four MFMAs per 32-key half, the exponentials,
// the stores.  No block-level synchronisation: the four LDS patches are private to their waves.  Per head the Q fragments are loaded once;
// under head_mean they are fetched per (key tile, head) from L2 (the heads' fragments of one wave would take 16 A registers), and the
// mean is a sum over the heads in the accumulators, divided by A.
template <bool F16, typename TO>
__global__ __launch_bounds__(256) void attn_probs_mfma_kernel(ProbArgs a) {
  __shared__ __attribute__((aligned(16))) char patches[4 * ATT_PATCH_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int tq, head0, b;
  att_block_at(a.order, tq, head0, b);
  const int L = a.L, H = a.H, ld = 3 * a.H, T = a.T;
  const int q0 = tq * 64 + 32 * (wid & 1), q = q0 + l31;
  if (q0 >= L) return;                       // a wave without queries (ragged last tile)
  const bool q_ok = q < L;
  uint8_t cl = 0;                            // tile classes of this query-tile row: lane t holds key tile t (T <= 64)
  if (lane < T) cl = a.info[((size_t)b * T + tq) * T + lane];
  const unsigned long long nz = __ballot(cl != 0), is1 = __ballot(cl == 1);
  const size_t rowbase = (size_t)b * L;
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.qkv, 0, a.bytes_qkv, 0x00020000);
  const float c2 = a.scale * LOG2E;
  const int nh = a.head_mean ? a.A : 1;
  bf16x8 qf[4];
  float lse2 = 0.f;
  auto load_q = [&](int head) {
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = load_rowfrag_global(rs, a.bytes_qkv, rowbase + q, q_ok, ld, head * 64 + 16 * s + 8 * h);
    lse2 = q_ok ? a.lse[((size_t)b * a.A + head) * L + q] * LOG2E : 0.f;
  };
  if (!a.head_mean) load_q(head0);
  const uint32_t* myw = a.bits + (rowbase + (q_ok ? q : 0)) * a.W;
  char* patch = patches + wid * ATT_PATCH_BYTES;
  const size_t plane = a.head_mean ? (size_t)b : (size_t)b * a.A + head0;
  TO* out = (TO*)a.out + (plane * L + q0) * (size_t)L;
  const int rows_ok = L - q0;
  for (int tk = wid >> 1; tk < T; tk += 2) {
    const int k0 = tk * 64;
    const int cls = ((is1 >> tk) & 1) ? 1 : (((nz >> tk) & 1) ? 2 : 0);
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
    if (cls != 0) {                           // class 0: the tile is written as zeros
      for (int hh = 0; hh < nh; ++hh) {
        const int head = a.head_mean ? hh : head0;
        if (a.head_mean) load_q(head);
        f32x16 st[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
          for (int i = 0; i < 16; ++i) st[kk][i] = 0.f;
          const int kr = k0 + 32 * kk + l31;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const bf16x8 kf = load_rowfrag_global(rs, a.bytes_qkv, rowbase + kr, kr < L, ld, H + head * 64 + 16 * s + 8 * h);
            st[kk] = mma32<F16>(kf, qf[s], st[kk]);
          }
        }
        const unsigned long long* mp =
            a.drop_on ? (const unsigned long long*)a.dropbits + ((((size_t)b * a.A + head) * (size_t)a.NQB + (q0 >> 5)) * (size_t)a.NKT + tk) * 32 : nullptr;
        if (cls == 1) probs_tile<false>(a, st, myw, q_ok, k0, c2, lse2, h, lane, mp);
        else probs_tile<true>(a, st, myw, q_ok, k0, c2, lse2, h, lane, mp);
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] += st[0][i]; acc[1][i] += st[1][i]; }
      }
      if (a.head_mean) {
        const float fa = (float)a.A;
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] /= fa; acc[1][i] /= fa; }
      }
    }
    probs_store_tile<TO>(patch, acc, out + k0, (size_t)L, rows_ok, L - k0, a.vec != 0, lane);
  }
}

// plain VALU form: one wave per (b, head -- or all heads --, query); the exact-fp32 path and the on-GPU cross-check of the MFMA kernel
template <typename T>
struct PSArgs {
  const T* qkv; const uint32_t* bits; const float* lse; void* out;
  int B, L, A, H, W, dh;
  float scale;
  const unsigned long long* dropbits;   // nullable = dropout off
  float inv_keep;
  int NQB, NKT;
  int head_mean;
};
template <typename T, typename TO>
__global__ __launch_bounds__(256) void attn_probs_simple_kernel(PSArgs<T> a) {
  __shared__ float sq[4][128];
  const int lane = threadIdx.x & 63, wl = threadIdx.x >> 6;
  const int AO = a.head_mean ? 1 : a.A;            // head planes of the output
  const long long wave = (long long)blockIdx.x * 4 + wl;
  if (wave >= (long long)a.B * AO * a.L) return;
  const int q = (int)(wave % a.L);
  const int ho = (int)((wave / a.L) % AO);
  const int b = (int)(wave / ((long long)a.L * AO));
  const int ld = 3 * a.H, dh = a.dh;
  const size_t rb = (size_t)b * a.L;
  const uint32_t* wrow = a.bits + (rb + q) * a.W;
  TO* orow = (TO*)a.out + (((size_t)b * AO + ho) * a.L + q) * (size_t)a.L;
  const int nh = a.head_mean ? a.A : 1;
  for (int k0 = 0; k0 < a.L; k0 += 64) {
    const int k = k0 + lane;
    float sum = 0.f;
    for (int hh = 0; hh < nh; ++hh) {
      const int hd = a.head_mean ? hh : ho;
      if (nh > 1 || k0 == 0) {
        __builtin_amdgcn_wave_barrier();
        const T* qp = a.qkv + (rb + q) * ld + hd * dh;
        for (int i = lane; i < dh; i += 64) sq[wl][i] = ldf<T>(qp + i);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      if (k < a.L) {
        const T* kp = a.qkv + (rb + k) * ld + a.H + hd * dh;
        float acc = 0.f;
        for (int i = 0; i < dh; ++i) acc = fmaf(sq[wl][i], ldf<T>(kp + i), acc);
        const float s = acc * a.scale + (((wrow[k >> 5] >> (k & 31)) & 1u) ? 0.f : MASK_ADD);
        float p = expf(s - a.lse[((size_t)b * a.A + hd) * a.L + q]);
        if (a.dropbits) p = attn_keep_bit(a.dropbits, a.NQB, a.NKT, (size_t)b * a.A + hd, q, k) ? p * a.inv_keep : 0.f;
        sum += p;
      }
    }
    if (k < a.L) stf<TO>(orow + k, a.head_mean ? sum / (float)a.A : sum);
  }
}

template <typename T, typename TO>
static int launch_simple_probs(const void* qkv, const uint32_t* bits, const float* lse, void* probs, int B, int L, int A, int dh, float p_drop,
                               const uint32_t* dropbits, int head_mean, hipStream_t stream) {
  PSArgs<T> s{};
  attn_fill_common(s, B, L, A, dh, p_drop, dropbits);
  s.qkv = (const T*)qkv; s.bits = bits; s.lse = lse; s.out = probs; s.head_mean = head_mean ? 1 : 0;
  s.dh = dh;
  const long long waves = (long long)B * (head_mean ? 1 : A) * L;
  hipLaunchKernelGGL((attn_probs_simple_kernel<T, TO>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, s);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_attn_probs(int dtype, const void* qkv, const uint32_t* bits, const uint8_t* tileinfo, const float* lse, void* probs,
                             int out_dtype, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits, int head_mean, void* stream_) {
  // (dtype of qkv, out_dtype): f32 probabilities, or qkv's encoding -- any other out_dtype is MV_E_ARG, refused below
  typedef mv_pairs<mv_pair<float, float>, mv_pair<bf16_t, float>, mv_pair<bf16_t, bf16_t>, mv_pair<f16_t, float>, mv_pair<f16_t, f16_t>> Accept;
  hipStream_t stream = (hipStream_t)stream_;
  if (!qkv || !bits || !tileinfo || !lse || !probs || B <= 0 || L <= 0 || A <= 0 || dh <= 0) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if (out_dtype != MV_F32 && out_dtype != dtype) return MV_E_ARG;      // f32, or the encoding of qkv
  const int Tt = (L + 63) / 64;
  if (Tt > 64) return MV_E_SHAPE;                                      // one lane per key tile's class, as in mv_mask_pack
  const int rcd = dropbits_check(p_drop, dropbits, B, L, A);
  if (rcd) return rcd;
  if ((((uintptr_t)qkv) & 15) || (((uintptr_t)probs) & 15)) return MV_E_SHAPE;
  const int H = A * dh;
  const bool o32 = out_dtype == MV_F32;
  if (mv_is16(dtype) && g_mv_impl == 0) {
    if (dh != 64) return MV_E_SHAPE;
    const size_t bq = (size_t)B * L * 3 * H * 2;
    if (bq >= 0x7fffffffULL) return MV_E_SHAPE;                        // qkv is read through a buffer descriptor (32-bit offsets)
    ProbArgs a{};
    attn_fill_common(a, B, L, A, dh, p_drop, dropbits);
    a.qkv = (const bf16_t*)qkv; a.bits = bits; a.info = tileinfo; a.lse = lse; a.out = probs;     // probs: plain 64-bit addressing
    a.T = Tt;
    a.bytes_qkv = (unsigned)bq;
    a.drop_on = p_drop > 0.f;
    a.head_mean = head_mean ? 1 : 0;
    a.vec = (L % (o32 ? 4 : 8)) == 0;
    a.order = mv_knob(MV_KNOB_ATTN_ORDER);
    const dim3 grid(Tt, head_mean ? 1 : A, B);
    return mv_with_types(dtype, out_dtype, Accept{}, [&](auto t, auto to) -> int {      // (f32 qkv never comes here: mv_is16 above)
      hipLaunchKernelGGL((attn_probs_mfma_kernel<decltype(t)::code == MV_F16, MV_T(to)>), grid, dim3(256), 0, stream, a);
      return (int)hipGetLastError();
    });
  }
  if (dh > 128) return MV_E_SHAPE;
  return mv_with_types(dtype, out_dtype, Accept{}, [&](auto t, auto to) {
    return launch_simple_probs<MV_T(t), MV_T(to)>(qkv, bits, lse, probs, B, L, A, dh, p_drop, dropbits, head_mean, stream);
  });
}
