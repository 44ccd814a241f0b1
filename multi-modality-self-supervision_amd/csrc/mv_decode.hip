// Report-generation decode path (KV-cached, UniLM scheme; DESIGN.md "Generation"): the kernels of one decode step that the
// pretraining kernels do not cover -- a weight-streaming GEMM for a few rows, attention of a few new queries against a slot
// cache, the fused log-softmax + top-k of the MLM head's rows and the embedding of single token rows.
//
//   mv_gemm_rows     y[M,N] = epi(x[M,K] . W[N,K]^T), M <= 256, 16-bit operands, MFMA 16x16x32, f32 accumulation
//   mv_attn_decode   ctx[r, head] = softmax(q k^T / sqrt(dh)) v over the cache slots listed for query row r; split-KV + lse merge
//   mv_logprob_topk  row log-softmax (f32) and its top-k (k <= 16, ties to the lower index), optional EOS column := -10000
//   mv_embed_rows    x[r] = LN(E[id] + Ty[seg] + P[pos])  (HF BertEmbeddings for one token row)
//   mv_ngram_ban     one beam step of n-gram blocking: gather the parents' word histories, append the chosen word, list the words
//                    that would repeat an n-gram
//   mv_logprob_topk_banned   mv_logprob_topk with -10000 added to the log-prob of every listed word of the row
#include "mv_dispatch.h"
#include "mv_gemm_common.h"

// ------------------------------------------------------------------------------------------------ mv_gemm_rows
// Block = 4 waves = one strip of 16 output columns (16 weight rows) over all M rows.  The 4 waves split the contraction in four
// contiguous ranges; each wave streams its 16 weight rows straight into VGPRs (the weights are read once, nothing is shared
// across waves: no LDS round trip) and multiplies every 16-row tile of x against them (x is small and L2-resident).  The four
// partial [M x 16] tiles are summed through LDS and the epilogue runs on the sum.  Lane l of a 16x16x32 MFMA holds operand row
// l & 15, k-chunk l >> 4 (8 values); the result lane holds D[4*(l>>4) + i][l & 15] with D rows from the first operand (weights,
// n) and columns from the second (x, m) -- the layout mv_gemm.hip's tile kernel relies on.
#define GR_WAVES 4
#define GR_BN 16
#define GR_LDR 16      // LDS row stride (floats) of the partial tiles: at M = 256 the four of them fill 64 KiB

template <bool F16, int MT, int CT>
__global__ __launch_bounds__(256) void gemm_rows_kernel(const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ W, int ldw,
                                                       void* __restrict__ c, int ldc, const float* __restrict__ bias, int epi,
                                                       const void* __restrict__ r, int ldr, int r_dtype, int M, int N, int K) {
  extern __shared__ float red[];               // [GR_WAVES][MT*16][GR_LDR]
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int n0 = blockIdx.x * GR_BN;
  const int nsteps = K >> 5;                   // K % 32 == 0 (checked by the host)
  const int s0 = wid * nsteps / GR_WAVES, s1 = (wid + 1) * nsteps / GR_WAVES;
  const int nrow = min(n0 + l15, N - 1);       // rows past N read row N-1 (in bounds); their columns are never stored
  const bf16_t* wp = W + (size_t)nrow * ldw + lq * 8;
  const bf16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) xp[t] = x + (size_t)min(t * 16 + l15, M - 1) * ldx + lq * 8;
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int U = 4;                         // weight fragments in flight per wave
  int s = s0;
  for (; s + U <= s1; s += U) {
    bf16x8 wf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) wf[u] = __builtin_nontemporal_load((const bf16x8*)(wp + (size_t)(s + u) * 32));
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const bf16x8 xf = *(const bf16x8*)(xp[t] + (size_t)(s + u) * 32);
        acc[t] = mma16<F16>(wf[u], xf, acc[t]);
      }
    }
  }
  for (; s < s1; ++s) {
    const bf16x8 wf = __builtin_nontemporal_load((const bf16x8*)(wp + (size_t)s * 32));
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = mma16<F16>(wf, *(const bf16x8*)(xp[t] + (size_t)s * 32), acc[t]);
  }
  // partial tile of this wave: D[n = 4*lq + i][m = t*16 + l15] -> red[wid][m][n]
  float* mine = red + (size_t)wid * (MT * 16) * GR_LDR;
#pragma unroll
  for (int t = 0; t < MT; ++t) *(f32x4*)(mine + (t * 16 + l15) * GR_LDR + 4 * lq) = acc[t];
  __syncthreads();
  // epilogue: thread -> (m, 4 consecutive columns)
  for (int g = tid; g < MT * 16 * 4; g += 256) {
    const int m = g >> 2, nl = (g & 3) * 4, n = n0 + nl;
    if (m >= M || n >= N) continue;
    f32x4 v = *(const f32x4*)(red + m * GR_LDR + nl);
#pragma unroll
    for (int w = 1; w < GR_WAVES; ++w) v += *(const f32x4*)(red + ((size_t)w * MT * 16 + m) * GR_LDR + nl);
    const int nv = min(4, N - n);
    for (int i = 0; i < nv; ++i) {
      float o = v[i];
      if (epi != MV_EPI_NONE) o += bias[n + i];
      if (epi == MV_EPI_BIAS_GELU) o = gelu_erf(o);
      else if (epi == MV_EPI_BIAS_RELU) o = fmaxf(o, 0.f);
      else if (epi == MV_EPI_BIAS_RES) o += ld_any(r, (size_t)m * ldr + n + i, r_dtype);
      v[i] = o;
    }
    if (CT == MV_F32) {
      float* cp = (float*)c + (size_t)m * ldc + n;
      if (nv == 4 && ((((uintptr_t)cp) & 15) == 0)) *(f32x4*)cp = v;
      else for (int i = 0; i < nv; ++i) cp[i] = v[i];
    } else if (CT == MV_F16) {
      f16_t* cp = (f16_t*)c + (size_t)m * ldc + n;
      if (nv == 4 && ((((uintptr_t)cp) & 7) == 0)) st4<f16_t>(cp, v);
      else for (int i = 0; i < nv; ++i) cp[i] = (f16_t)v[i];
    } else {
      bf16_t* cp = (bf16_t*)c + (size_t)m * ldc + n;
      if (nv == 4 && ((((uintptr_t)cp) & 7) == 0)) st4<bf16_t>(cp, v);
      else for (int i = 0; i < nv; ++i) cp[i] = (bf16_t)v[i];
    }
  }
}

template <bool F16>
static int launch_gemm_rows(int mt, int c_dtype, dim3 grid, hipStream_t st, const bf16_t* x, int ldx, const bf16_t* W, int ldw, void* c,
                            int ldc, const float* bias, int epi, const void* r, int ldr, int r_dtype, int M, int N, int K) {
  const size_t lds = (size_t)GR_WAVES * mt * 16 * GR_LDR * sizeof(float);
  return mv_with_type(c_dtype, [&](auto tc) -> int {      // every output encoding, for either 16-bit operand encoding
    constexpr int CT = decltype(tc)::code;
#define GR_CASE(T_) \
  case T_: hipLaunchKernelGGL((gemm_rows_kernel<F16, T_, CT>), grid, dim3(256), lds, st, x, ldx, W, ldw, c, ldc, bias, epi, r, ldr, r_dtype, M, N, K); break;
    switch (mt) {
      GR_CASE(1) GR_CASE(2) GR_CASE(3) GR_CASE(4) GR_CASE(5) GR_CASE(6) GR_CASE(7) GR_CASE(8)
      GR_CASE(9) GR_CASE(10) GR_CASE(11) GR_CASE(12) GR_CASE(13) GR_CASE(14) GR_CASE(15) GR_CASE(16)
    }
#undef GR_CASE
    return (int)hipGetLastError();
  });
}

extern "C" int mv_gemm_rows(int dtype, int M, int N, int K, const void* x, int ldx, const void* W, int ldw, void* c, int ldc, int c_dtype,
                            const float* bias, int epi, const void* r, int ldr, int r_dtype, void* stream_) {
  typedef mv_types<bf16_t, f16_t> Accept;      // of x and W; c_dtype is any of the three (launch_gemm_rows)
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !W || !c || M <= 0 || N <= 0 || K <= 0) return MV_E_ARG;
  if (!mv_is16(dtype) || !mv_dtype_ok(c_dtype)) return MV_E_DTYPE;
  if (epi != MV_EPI_NONE && epi != MV_EPI_BIAS && epi != MV_EPI_BIAS_GELU && epi != MV_EPI_BIAS_RES && epi != MV_EPI_BIAS_RELU)
    return MV_E_ARG;
  if (epi != MV_EPI_NONE && !bias) return MV_E_ARG;
  if (epi == MV_EPI_BIAS_RES && (!r || !mv_dtype_ok(r_dtype) || ldr < N)) return MV_E_ARG;
  if (M > 256 || (K & 31) || (ldx & 7) || (ldw & 7) || ldx < K || ldw < K || ldc < N) return MV_E_SHAPE;
  if ((((uintptr_t)x) & 15) || (((uintptr_t)W) & 15)) return MV_E_SHAPE;
  const int mt = (M + 15) / 16;
  dim3 grid((N + GR_BN - 1) / GR_BN);
  return mv_with_type(dtype, Accept{}, [&](auto t) {      // the kernel takes both operand encodings as bf16_t pointers; F16 picks the MFMA
    return launch_gemm_rows<decltype(t)::code == MV_F16>(mt, c_dtype, grid, stream, (const bf16_t*)x, ldx, (const bf16_t*)W, ldw, c, ldc, bias, epi,
                                                            r, ldr, r_dtype, M, N, K);
  });
}

// ------------------------------------------------------------------------------------------------ mv_attn_decode
// Block = (query row r, head h, split s): 256 threads walk the split's share of the row's key list in tiles of 256 keys -- one
// key per thread for the score (q . k, f32), an online softmax over the tiles (running max / sum), then the tile's p.V with
// thread -> (key group g, column d): consecutive lanes read consecutive columns of one value row.  One split writes the
// normalised context; several write (unnormalised context, max, sum) partials that attn_decode_merge combines (flash-decoding).
template <typename T>
__device__ __forceinline__ float dot_row(const float* __restrict__ qs, const T* __restrict__ kr, int dh) {
  float s = 0.f;
  for (int d = 0; d < dh; d += 4) {
    const f32x4 k4 = ld4<T>(kr + d);
    s += qs[d] * k4[0] + qs[d + 1] * k4[1] + qs[d + 2] * k4[2] + qs[d + 3] * k4[3];
  }
  return s;
}

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int wid = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[wid] = v;
  __syncthreads();
  float o = sh[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) o = is_max ? fmaxf(o, sh[w]) : o + sh[w];
  return o;
}

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ kc, const T* __restrict__ vc,
                                                         int ldkv, const int32_t* __restrict__ slots, int ld_slots,
                                                         const int32_t* __restrict__ slot_row, const int32_t* __restrict__ nk,
                                                         T* __restrict__ ctx, int ldo, float* __restrict__ ws, int A, int dh, int nsplit,
                                                         float scale) {
  __shared__ float qs[128];
  __shared__ float ps[256];
  __shared__ int ss[256];
  __shared__ float sh[4];
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int r = blockIdx.x / A, h = blockIdx.x - r * A, sp = blockIdx.y;
  const int n = nk[r];
  const int chunk = (n + nsplit - 1) / nsplit;
  const int j0 = sp * chunk, j1 = min(n, j0 + chunk);
  const int32_t* sl = slots + (size_t)(slot_row ? slot_row[r] : r) * ld_slots;
  if (tid < dh) qs[tid] = ldf<T>(q + (size_t)r * ldq + h * dh + tid) * scale;
  const int G = 256 / dh, g = tid / dh, d = tid - g * dh;
  float m_run = -INFINITY, l_run = 0.f, acc = 0.f;
  __syncthreads();
  for (int jt = j0; jt < j1; jt += 256) {
    const int j = jt + tid;
    float sc = -INFINITY;
    int slot = 0;
    if (j < j1) {
      slot = sl[j];
      sc = dot_row<T>(qs, kc + (size_t)slot * ldkv + h * dh, dh);
    }
    const float tmax = block_reduce(sc, sh, true);
    const float m_new = fmaxf(m_run, tmax);
    const float p = (j < j1) ? __expf(sc - m_new) : 0.f;
    ps[tid] = p;
    ss[tid] = slot;
    const float tsum = block_reduce(p, sh, false);      // (its barriers also publish ps / ss)
    const float corr = __expf(m_run - m_new);            // m_run = -inf on the first tile: 0
    l_run = l_run * corr + tsum;
    acc *= corr;
    m_run = m_new;
    const int cnt = min(256, j1 - jt);
    const T* vcol = vc + h * dh + d;
    for (int jj = g; jj < cnt; jj += G) acc += ps[jj] * ldf<T>(vcol + (size_t)ss[jj] * ldkv);
    __syncthreads();                                     // ps / ss are rewritten by the next tile
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < dh) {
    float o = 0.f;
    for (int k = 0; k < G; ++k) o += red[k * dh + tid];
    if (nsplit == 1) {
      stf<T>(ctx + (size_t)r * ldo + h * dh + tid, l_run > 0.f ? o / l_run : 0.f);
    } else {
      float* w = ws + ((size_t)blockIdx.x * nsplit + sp) * (dh + 2);
      w[2 + tid] = o;
      if (tid == 0) { w[0] = m_run; w[1] = l_run; }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(128) void attn_decode_merge(const float* __restrict__ ws, T* __restrict__ ctx, int ldo, int A, int dh, int nsplit) {
  const int rh = blockIdx.x, r = rh / A, h = rh - r * A, d = threadIdx.x;
  if (d >= dh) return;
  const float* w = ws + (size_t)rh * nsplit * (dh + 2);
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, w[(size_t)s * (dh + 2)]);
  float l = 0.f, o = 0.f;
  if (M > -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float* ws_ = w + (size_t)s * (dh + 2);
      const float e = __expf(ws_[0] - M);               // an empty split (max -inf) weighs 0
      l += ws_[1] * e;
      o += ws_[2 + d] * e;
    }
  }
  stf<T>(ctx + (size_t)r * ldo + h * dh + d, l > 0.f ? o / l : 0.f);
}

// split count when the caller leaves it to the library: enough (row, head, split) blocks for two per CU, at least 128 keys per
// split, as many as the workspace holds
static int decode_splits(int R, int A, int dh, int max_nk, size_t ws_floats) {
  const int pairs = R * A;
  int s = (512 + pairs - 1) / pairs;
  s = min(s, max(1, (max_nk + 127) / 128));
  s = min(s, 32);
  while (s > 1 && (size_t)s * pairs * (dh + 2) > ws_floats) --s;
  return max(s, 1);
}

extern "C" int mv_attn_decode(int dtype, const void* q, int ldq, const void* k_cache, const void* v_cache, int ldkv, const int32_t* slots,
                              int ld_slots, const int32_t* slot_row, const int32_t* nk, int max_nk, void* ctx, int ldo, int R, int A, int dh,
                              int nsplit, float* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!q || !k_cache || !v_cache || !slots || !nk || !ctx || R <= 0 || A <= 0 || dh <= 0 || max_nk <= 0 || nsplit < 0) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if (dh > 128 || (256 % dh) || (dh & 3) || (ldq & 3) || (ldkv & 3) || ldq < A * dh || ldkv < A * dh || ldo < A * dh || ld_slots < 1)
    return MV_E_SHAPE;
  const size_t ws_floats = ws ? ws_bytes / sizeof(float) : 0;
  int ns = nsplit == 0 ? decode_splits(R, A, dh, max_nk, ws_floats) : nsplit;
  if (ns > 1 && (size_t)ns * R * A * (dh + 2) > ws_floats) return MV_E_WORKSPACE;
  const float scale = 1.0f / sqrtf((float)dh);
  dim3 grid(R * A, ns);
  return mv_with_type(dtype, [&](auto t) -> int {
    typedef MV_T(t) T;
    hipLaunchKernelGGL(attn_decode_kernel<T>, grid, dim3(256), 0, stream, (const T*)q, ldq, (const T*)k_cache, (const T*)v_cache, ldkv, slots, ld_slots,
                       slot_row, nk, (T*)ctx, ldo, ws, A, dh, ns, scale);
    MV_CHECK_LAUNCH();
    if (ns > 1) hipLaunchKernelGGL(attn_decode_merge<T>, dim3(R * A), dim3(128), 0, stream, (const float*)ws, (T*)ctx, ldo, A, dh, ns);
    return (int)hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------------------ mv_logprob_topk
// Block = one row.  Each thread scans a strided share of the columns once: running (max, sum of exp) for the log-sum-exp and a
// sorted list of its KM best (value desc, index asc).  The row's top-k is then k rounds of a block-wide argmax over the heads
// of the lists; the winner pops its head.  The EOS column (when penalised) stays in the log-sum-exp and enters the selection
// with the log-prob -10000 exactly, as the reference's fill_ after log_softmax.
__device__ __forceinline__ bool tk_better(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

template <int KM>
__device__ __forceinline__ void tk_insert(float (&v)[KM], int (&ix)[KM], float x, int c) {
#pragma unroll
  for (int i = 0; i < KM; ++i) {
    if (tk_better(x, c, v[i], ix[i])) {
      const float tv = v[i];
      const int ti = ix[i];
      v[i] = x;
      ix[i] = c;
      x = tv;
      c = ti;
    }
  }
}

template <int KM>
__global__ __launch_bounds__(256) void logprob_topk_kernel(const float* __restrict__ logits, int ld, int V, int k, int eos,
                                                          float* __restrict__ vals, int64_t* __restrict__ idx, float* __restrict__ lse_out) {
  __shared__ float shm[4], shs[4], shv[4];
  __shared__ int shi[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* x = logits + (size_t)row * ld;
  float v[KM];
  int ix[KM];
#pragma unroll
  for (int i = 0; i < KM; ++i) { v[i] = -INFINITY; ix[i] = 0x7fffffff; }
  float m = -INFINITY, s = 0.f;
  for (int c = tid; c < V; c += 256) {
    const float xv = x[c];
    if (xv > m) { s = s * __expf(m - xv) + 1.f; m = xv; }
    else if (xv > -INFINITY) s += __expf(xv - m);       // a -inf logit adds nothing (with m still -inf, xv - m would be NaN)
    if (c != eos) tk_insert<KM>(v, ix, xv, c);
  }
  // log-sum-exp of the row
  float bm = wave_max(m);
  if (lane == 0) shm[wid] = bm;
  __syncthreads();
  bm = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
  float bs = wave_sum(m > -INFINITY ? s * __expf(m - bm) : 0.f);
  if (lane == 0) shs[wid] = bs;
  __syncthreads();
  const float lse = bm + __logf(shs[0] + shs[1] + shs[2] + shs[3]);
  if (eos >= 0 && eos < V && tid == (eos & 255)) tk_insert<KM>(v, ix, -10000.0f + lse, eos);
  for (int o = 0; o < k; ++o) {
    float bv = v[0];
    int bi = ix[0];
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { shv[wid] = bv; shi[wid] = bi; }
    __syncthreads();
    bv = shv[0];
    bi = shi[0];
    for (int w = 1; w < 4; ++w)
      if (tk_better(shv[w], shi[w], bv, bi)) { bv = shv[w]; bi = shi[w]; }
    if (ix[0] == bi) {                              // the owner pops its head
#pragma unroll
      for (int i = 0; i + 1 < KM; ++i) { v[i] = v[i + 1]; ix[i] = ix[i + 1]; }
      v[KM - 1] = -INFINITY;
      ix[KM - 1] = 0x7fffffff;
    }
    if (tid == 0) {
      vals[(size_t)row * k + o] = (bi == eos) ? -10000.0f : bv - lse;
      idx[(size_t)row * k + o] = bi;
    }
  }
  if (lse_out && tid == 0) lse_out[row] = lse;
}

extern "C" int mv_logprob_topk(const float* logits, int ld, int R, int V, int k, int eos_penalty_id, float* vals, int64_t* idx, float* lse,
                               void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !vals || !idx || R <= 0 || V <= 0 || ld < V || k <= 0) return MV_E_ARG;
  if (k > 16 || k > V) return MV_E_SHAPE;
  const int eos = (eos_penalty_id >= 0 && eos_penalty_id < V) ? eos_penalty_id : -1;
  if (k == 1) hipLaunchKernelGGL(logprob_topk_kernel<1>, dim3(R), dim3(256), 0, stream, logits, ld, V, k, eos, vals, idx, lse);
  else if (k <= 4) hipLaunchKernelGGL(logprob_topk_kernel<4>, dim3(R), dim3(256), 0, stream, logits, ld, V, k, eos, vals, idx, lse);
  else hipLaunchKernelGGL(logprob_topk_kernel<16>, dim3(R), dim3(256), 0, stream, logits, ld, V, k, eos, vals, idx, lse);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

// ------------------------------------------------------------------------------------------------ mv_embed_rows
// Block = one row: x = LN(E[id] + Ty[seg] + P[pos]) in f32, written in `dtype`.  Indices are clamped into their tables.
template <typename T>
__global__ __launch_bounds__(256) void embed_rows_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos,
                                                        const int64_t* __restrict__ seg, const T* __restrict__ E, const T* __restrict__ P,
                                                        const T* __restrict__ Ty, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, T* __restrict__ out, int ldo, int H, int V, int maxpos,
                                                        int ntype, float eps) {
  __shared__ float sh[4];
  extern __shared__ float rowv[];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long long id = min(max(ids[r], (int64_t)0), (int64_t)V - 1);
  const long long p = min(max(pos[r], (int64_t)0), (int64_t)maxpos - 1);
  const long long t = min(max(seg[r], (int64_t)0), (int64_t)ntype - 1);
  float s = 0.f;
  for (int c = tid; c < H; c += 256) {
    const float e = ldf<T>(E + id * H + c) + ldf<T>(Ty + t * H + c) + ldf<T>(P + p * H + c);
    rowv[c] = e;
    s += e;
  }
  const float mean = block_reduce(s, sh, false) / H;
  float q = 0.f;
  for (int c = tid; c < H; c += 256) {
    const float dv = rowv[c] - mean;
    q += dv * dv;
  }
  const float rstd = rsqrtf(block_reduce(q, sh, false) / H + eps);
  for (int c = tid; c < H; c += 256) stf<T>(out + (size_t)r * ldo + c, (rowv[c] - mean) * rstd * gamma[c] + beta[c]);
}

extern "C" int mv_embed_rows(int dtype, const int64_t* ids, const int64_t* pos, const int64_t* seg, const void* E, const void* P, const void* Ty,
                             const float* gamma, const float* beta, void* out, int ldo, int R, int H, int V, int maxpos, int ntype, float eps,
                             void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ids || !pos || !seg || !E || !P || !Ty || !gamma || !beta || !out || R <= 0 || H <= 0 || V <= 0 || maxpos <= 0 || ntype <= 0)
    return MV_E_ARG;
  if (ldo < H || H > 8192) return MV_E_SHAPE;
  const size_t lds = (size_t)H * sizeof(float);
  return mv_with_type(dtype, [&](auto t) -> int {
    typedef MV_T(t) T;
    hipLaunchKernelGGL(embed_rows_kernel<T>, dim3(R), dim3(256), lds, stream, ids, pos, seg, (const T*)E, (const T*)P, (const T*)Ty, gamma, beta,
                       (T*)out, ldo, H, V, maxpos, ntype, eps);
    return (int)hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------------------ mv_ngram_ban
// Block = one beam.  The beam's new history (its parent's words, then the word just chosen) is staged in LDS and written out; every
// window of n - 1 words is compared with the last n - 1 (the tail), the word behind a matching window is a candidate.  Candidates
// are few: the duplicates are dropped and the rest ranked by counting, so the list comes out ascending without a sort network.
#define NB_MAX_LEN 1024      // words of one history, the new one included
#define NB_MAX_IGN 256       // ignore ids
#define NB_MIN_N 2
#define NB_MAX_N 8

__global__ __launch_bounds__(256) void ngram_ban_kernel(const int32_t* __restrict__ hist_in, int32_t* __restrict__ hist_out, int ld_h,
                                                       const int64_t* __restrict__ parent, const int64_t* __restrict__ y, int R, int len,
                                                       int n, const int32_t* __restrict__ ignore, int n_ign, int32_t* __restrict__ ban,
                                                       int ld_ban, int32_t* __restrict__ nban) {
  __shared__ int32_t seq[NB_MAX_LEN];
  __shared__ int32_t cand[NB_MAX_LEN];
  __shared__ int32_t keep[NB_MAX_LEN];
  __shared__ int32_t ign[NB_MAX_IGN];
  __shared__ int count;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int L = len + 1;                               // words of the new history
  long long p = parent ? (long long)parent[r] : r;
  p = min(max(p, 0ll), (long long)R - 1);              // a parent outside [0, R) reads the first / last row
  const int32_t* src = hist_in + (size_t)p * ld_h;
  int32_t* dst = hist_out + (size_t)r * ld_h;
  for (int i = tid; i < L; i += 256) {
    const int32_t w = i < len ? src[i] : (int32_t)y[r];
    seq[i] = w;
    dst[i] = w;
  }
  for (int i = tid; i < n_ign; i += 256) ign[i] = ignore[i];
  if (tid == 0) count = 0;
  __syncthreads();
  const int W = L - n + 1;                             // windows of n - 1 words that have a word behind them
  if (W <= 0) {                                        // fewer than n words: nothing is banned
    if (tid == 0) nban[r] = 0;
    return;
  }
  const int32_t* tail = seq + L - (n - 1);
  int hit = 0;                                         // an ignore word in the tail switches the rule off for this beam
  if (tid < n - 1)
    for (int j = 0; j < n_ign; ++j) hit |= (ign[j] == tail[tid]);
  if (__syncthreads_or(hit)) {
    if (tid == 0) nban[r] = 0;
    return;
  }
  for (int i = tid; i < W; i += 256) {
    bool ok = true;
    for (int j = 0; j < n - 1; ++j) ok &= (seq[i + j] == tail[j]);
    const int32_t w = seq[i + n - 1];
    if (ok)
      for (int j = 0; j < n_ign; ++j) ok &= (ign[j] != w);
    cand[i] = ok ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < W; i += 256) {                 // a word several windows ban counts at its first window
    int first = cand[i];
    if (first) {
      const int32_t w = seq[i + n - 1];
      for (int j = 0; j < i; ++j) first &= !(cand[j] && seq[j + n - 1] == w);
    }
    keep[i] = first;
  }
  __syncthreads();
  for (int i = tid; i < W; i += 256) {
    if (!keep[i]) continue;
    const int32_t w = seq[i + n - 1];
    int rank = 0;
    for (int j = 0; j < W; ++j) rank += (keep[j] && seq[j + n - 1] < w);
    if (rank < ld_ban) ban[(size_t)r * ld_ban + rank] = w;        // rank < W <= ld_ban (checked by the host)
    atomicAdd(&count, 1);
  }
  __syncthreads();
  if (tid == 0) nban[r] = count;
}

extern "C" int mv_ngram_ban(const int32_t* hist_in, int32_t* hist_out, int ld_h, const int64_t* parent, const int64_t* y, int R, int len,
                            int n, const int32_t* ignore, int n_ign, int32_t* ban, int ld_ban, int32_t* nban, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!hist_in || !hist_out || !y || !ban || !nban || R <= 0 || len < 0 || ld_h <= 0 || ld_ban < 0 || n_ign < 0) return MV_E_ARG;
  if (n < NB_MIN_N || n > NB_MAX_N) return MV_E_ARG;
  if (n_ign > 0 && !ignore) return MV_E_ARG;
  if (len + 1 > NB_MAX_LEN || n_ign > NB_MAX_IGN) return MV_E_SHAPE;
  if (ld_h < len + 1 || ld_ban < len + 2 - n) return MV_E_SHAPE;
  {                                                    // the gather reads rows the same launch writes: the two histories must not overlap
    const uintptr_t a = (uintptr_t)hist_in, b = (uintptr_t)hist_out;
    const uintptr_t span = ((size_t)(R - 1) * ld_h + len + 1) * sizeof(int32_t);
    if (a < b + span && b < a + span) return MV_E_ARG;
  }
  hipLaunchKernelGGL(ngram_ban_kernel, dim3(R), dim3(256), 0, stream, hist_in, hist_out, ld_h, parent, y, R, len, n, ignore, n_ign, ban,
                     ld_ban, nban);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

// ------------------------------------------------------------------------------------------------ mv_logprob_topk_banned
// mv_logprob_topk's block with the row's banned words marked in an LDS bitmap over the vocabulary.  The scan keeps banned columns
// out of the per-thread lists (as it keeps the penalised EOS column out); once the log-sum-exp is known they enter with their final
// value fl(fl(x - lse) - 10000).  List entries of banned columns carry ~column (negative) and their value is a log-prob; all other
// entries are raw logits as in mv_logprob_topk.  Two unbanned entries compare as there, so a row without bans selects bit for bit
// what mv_logprob_topk selects; a comparison that involves a banned entry is made on the final values (ties to the lower column).
#define TKB_MAX_V 131072     // bitmap: one bit per column, 16 KiB of LDS

__device__ __forceinline__ bool tkb_better(float va, int ia, float vb, int ib, float lse, int eos) {
  if ((ia | ib) >= 0) return tk_better(va, ia, vb, ib);
  const float fa = ia < 0 ? va : (ia == eos ? -10000.0f : va - lse), fb = ib < 0 ? vb : (ib == eos ? -10000.0f : vb - lse);
  const int ca = ia < 0 ? ~ia : ia, cb = ib < 0 ? ~ib : ib;
  return fa > fb || (fa == fb && ca < cb);
}

template <int KM>
__device__ __forceinline__ void tkb_insert(float (&v)[KM], int (&ix)[KM], float x, int c, float lse, int eos) {
#pragma unroll
  for (int i = 0; i < KM; ++i) {
    if (tkb_better(x, c, v[i], ix[i], lse, eos)) {
      const float tv = v[i];
      const int ti = ix[i];
      v[i] = x;
      ix[i] = c;
      x = tv;
      c = ti;
    }
  }
}

template <int KM>
__global__ __launch_bounds__(256) void logprob_topk_banned_kernel(const float* __restrict__ logits, int ld, int V, int k, int eos,
                                                                 const int32_t* __restrict__ ban, int ld_ban, const int32_t* __restrict__ nban,
                                                                 float* __restrict__ vals, int64_t* __restrict__ idx, float* __restrict__ lse_out) {
  extern __shared__ unsigned bits[];                 // [(V + 31) / 32]
  __shared__ float shm[4], shs[4], shv[4];
  __shared__ int shi[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* x = logits + (size_t)row * ld;
  const int nb = ban ? min(max(nban[row], 0), ld_ban) : 0;
  const int nwords = (V + 31) >> 5;
  if (nb > 0) {                                      // (block-uniform)
    for (int w = tid; w < nwords; w += 256) bits[w] = 0u;
    __syncthreads();
    for (int j = tid; j < nb; j += 256) {
      const int c = ban[(size_t)row * ld_ban + j];
      if (c >= 0 && c < V) atomicOr(&bits[c >> 5], 1u << (c & 31));          // ids outside the vocabulary are ignored
    }
    __syncthreads();
  }
  float v[KM];
  int ix[KM];
#pragma unroll
  for (int i = 0; i < KM; ++i) { v[i] = -INFINITY; ix[i] = 0x7fffffff; }
  float m = -INFINITY, s = 0.f;
  for (int c = tid; c < V; c += 256) {
    const float xv = x[c];
    if (xv > m) { s = s * __expf(m - xv) + 1.f; m = xv; }
    else if (xv > -INFINITY) s += __expf(xv - m);
    const bool banned = nb > 0 && ((bits[c >> 5] >> (c & 31)) & 1u);
    if (c != eos && !banned) tk_insert<KM>(v, ix, xv, c);
  }
  float bm = wave_max(m);
  if (lane == 0) shm[wid] = bm;
  __syncthreads();
  bm = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
  float bs = wave_sum(m > -INFINITY ? s * __expf(m - bm) : 0.f);
  if (lane == 0) shs[wid] = bs;
  __syncthreads();
  const float lse = bm + __logf(shs[0] + shs[1] + shs[2] + shs[3]);
  if (eos >= 0 && eos < V && tid == (eos & 255)) tk_insert<KM>(v, ix, -10000.0f + lse, eos);
  if (nb > 0) {
    for (int w = tid; w < nwords; w += 256) {        // every marked column once, whatever the list held twice
      unsigned b = bits[w];
      while (b) {
        const int c = (w << 5) + __ffs((int)b) - 1;
        b &= b - 1;
        if (c == eos) continue;                      // banned and penalised: -10000 exactly, entered above
        const float lp = x[c] - lse;
        tkb_insert<KM>(v, ix, lp + -10000.0f, ~c, lse, eos);
      }
    }
  }
  for (int o = 0; o < k; ++o) {
    float bv = v[0];
    int bi = ix[0];
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (tkb_better(ov, oi, bv, bi, lse, eos)) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { shv[wid] = bv; shi[wid] = bi; }
    __syncthreads();
    bv = shv[0];
    bi = shi[0];
    for (int w = 1; w < 4; ++w)
      if (tkb_better(shv[w], shi[w], bv, bi, lse, eos)) { bv = shv[w]; bi = shi[w]; }
    if (ix[0] == bi) {                              // the owner pops its head
#pragma unroll
      for (int i = 0; i + 1 < KM; ++i) { v[i] = v[i + 1]; ix[i] = ix[i + 1]; }
      v[KM - 1] = -INFINITY;
      ix[KM - 1] = 0x7fffffff;
    }
    if (tid == 0) {
      vals[(size_t)row * k + o] = bi < 0 ? bv : ((bi == eos) ? -10000.0f : bv - lse);
      idx[(size_t)row * k + o] = bi < 0 ? ~bi : bi;
    }
  }
  if (lse_out && tid == 0) lse_out[row] = lse;
}

extern "C" int mv_logprob_topk_banned(const float* logits, int ld, int R, int V, int k, int eos_penalty_id, const int32_t* ban, int ld_ban,
                                      const int32_t* nban, float* vals, int64_t* idx, float* lse, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !vals || !idx || R <= 0 || V <= 0 || ld < V || k <= 0) return MV_E_ARG;
  if (ban && (!nban || ld_ban <= 0)) return MV_E_ARG;
  if (k > 16 || k > V || V > TKB_MAX_V) return MV_E_SHAPE;
  const int eos = (eos_penalty_id >= 0 && eos_penalty_id < V) ? eos_penalty_id : -1;
  const size_t lds = ban ? (size_t)((V + 31) / 32) * sizeof(unsigned) : 0;
#define TKB_LAUNCH(KM_) \
  hipLaunchKernelGGL(logprob_topk_banned_kernel<KM_>, dim3(R), dim3(256), lds, stream, logits, ld, V, k, eos, ban, ld_ban, nban, vals, idx, lse)
  if (k == 1) TKB_LAUNCH(1);
  else if (k <= 4) TKB_LAUNCH(4);
  else TKB_LAUNCH(16);
#undef TKB_LAUNCH
  MV_CHECK_LAUNCH();
  return MV_OK;
}
