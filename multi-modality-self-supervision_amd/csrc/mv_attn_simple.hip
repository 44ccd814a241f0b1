// The plain VALU attention kernels (any encoding, dh <= 128) and their launchers.
#include "mv_attn.h"

// =========================================================================================
// plain VALU kernels (any dtype, dh <= 128): exact-fp32 path and cross-check
// =========================================================================================
template <typename T>
struct SArgs {
  const T* qkv; const T* ctx; const T* dctx; T* out; T* dqkv;
  const uint32_t* bits; float* lse; const float* lse_in; float* delta;
  int B, L, A, H, W, dh;
  float scale;
  const unsigned long long* dropbits;   // nullable = dropout off; layout of AttnArgs::dropbits
  float inv_keep;
  int NQB, NKT;
};

// delta[b,h,q] = sum_d dctx*ctx   (one wave per (b,q,h))
template <typename T>
__global__ void attn_delta_kernel(const T* __restrict__ ctx, const T* __restrict__ dctx, float* __restrict__ delta, int B, int L,
                                  int A, int H, int dh) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= B * L * A) return;
  const int hd = wave % A, row = wave / A;   // row = b*L + q
  const T* c = ctx + (size_t)row * H + hd * dh;
  const T* d = dctx + (size_t)row * H + hd * dh;
  float s = 0.f;
  for (int i = lane; i < dh; i += 64) s += ldf<T>(c + i) * ldf<T>(d + i);
  s = wave_sum(s);
  if (lane == 0) {
    const int b = row / L, q = row - b * L;
    delta[((size_t)b * A + hd) * L + q] = s;
  }
}

// one wave per (b, h, q)
template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_simple_kernel(SArgs<T> a) {
  __shared__ float sq[4][128];
  __shared__ float sp[4][64];
  const int lane = threadIdx.x & 63, wl = threadIdx.x >> 6;
  const long long wave = (long long)blockIdx.x * 4 + wl;
  if (wave >= (long long)a.B * a.A * a.L) return;
  const int q = (int)(wave % a.L);
  const int hd = (int)((wave / a.L) % a.A);
  const int b = (int)(wave / ((long long)a.L * a.A));
  const int ld = 3 * a.H, dh = a.dh;
  const size_t rb = (size_t)b * a.L;
  const T* qp = a.qkv + (rb + q) * ld + hd * dh;
  for (int i = lane; i < dh; i += 64) sq[wl][i] = ldf<T>(qp + i);
  float m = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f;
  const uint32_t* wrow = a.bits + (rb + q) * a.W;
  for (int k0 = 0; k0 < a.L; k0 += 64) {
    const int k = k0 + lane;
    float s = -INFINITY;
    if (k < a.L) {
      const T* kp = a.qkv + (rb + k) * ld + a.H + hd * dh;
      float acc = 0.f;
      for (int i = 0; i < dh; ++i) acc = fmaf(sq[wl][i], ldf<T>(kp + i), acc);
      s = acc * a.scale + (((wrow[k >> 5] >> (k & 31)) & 1u) ? 0.f : MASK_ADD);
    }
    const float mx = wave_max(s);
    const float mn = fmaxf(m, mx);
    const float alpha = expf(m - mn);
    const float p = (k < a.L) ? expf(s - mn) : 0.f;
    l = l * alpha + wave_sum(p);
    m = mn;
    float pd = p;
    if (a.dropbits && k < a.L) pd = attn_keep_bit(a.dropbits, a.NQB, a.NKT, (size_t)b * a.A + hd, q, k) ? p * a.inv_keep : 0.f;
    sp[wl][lane] = pd;
    o0 *= alpha; o1 *= alpha;
    const int kn = min(64, a.L - k0);
    for (int j = 0; j < kn; ++j) {
      const T* vp = a.qkv + (rb + k0 + j) * ld + 2 * a.H + hd * dh;
      const float pj = sp[wl][j];
      if (lane < dh) o0 = fmaf(pj, ldf<T>(vp + lane), o0);
      if (lane + 64 < dh) o1 = fmaf(pj, ldf<T>(vp + lane + 64), o1);
    }
  }
  T* op = a.out + (rb + q) * a.H + hd * dh;
  if (lane < dh) stf<T>(op + lane, o0 / l);
  if (lane + 64 < dh) stf<T>(op + lane + 64, o1 / l);
  if (lane == 0) a.lse[((size_t)b * a.A + hd) * a.L + q] = m + logf(l);
}

// dQ: one wave per (b,h,q)
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dq_simple_kernel(SArgs<T> a) {
  __shared__ float sq[4][128];
  __shared__ float sdo[4][128];
  __shared__ float sds[4][64];
  const int lane = threadIdx.x & 63, wl = threadIdx.x >> 6;
  const long long wave = (long long)blockIdx.x * 4 + wl;
  if (wave >= (long long)a.B * a.A * a.L) return;
  const int q = (int)(wave % a.L);
  const int hd = (int)((wave / a.L) % a.A);
  const int b = (int)(wave / ((long long)a.L * a.A));
  const int ld = 3 * a.H, dh = a.dh;
  const size_t rb = (size_t)b * a.L;
  const T* qp = a.qkv + (rb + q) * ld + hd * dh;
  const T* dop = a.dctx + (rb + q) * a.H + hd * dh;
  for (int i = lane; i < dh; i += 64) { sq[wl][i] = ldf<T>(qp + i); sdo[wl][i] = ldf<T>(dop + i); }
  const size_t si = ((size_t)b * a.A + hd) * a.L + q;
  const float lse = a.lse_in[si], dl = a.delta[si];
  const uint32_t* wrow = a.bits + (rb + q) * a.W;
  float g0 = 0.f, g1 = 0.f;
  for (int k0 = 0; k0 < a.L; k0 += 64) {
    const int k = k0 + lane;
    float ds = 0.f;
    if (k < a.L) {
      const T* kp = a.qkv + (rb + k) * ld + a.H + hd * dh;
      const T* vp = kp + a.H;
      float acc = 0.f, dp = 0.f;
      for (int i = 0; i < dh; ++i) { acc = fmaf(sq[wl][i], ldf<T>(kp + i), acc); dp = fmaf(sdo[wl][i], ldf<T>(vp + i), dp); }
      const float s = acc * a.scale + (((wrow[k >> 5] >> (k & 31)) & 1u) ? 0.f : MASK_ADD);
      if (a.dropbits) dp = attn_keep_bit(a.dropbits, a.NQB, a.NKT, (size_t)b * a.A + hd, q, k) ? dp * a.inv_keep : 0.f;
      ds = expf(s - lse) * (dp - dl) * a.scale;
    }
    sds[wl][lane] = ds;
    const int kn = min(64, a.L - k0);
    for (int j = 0; j < kn; ++j) {
      const T* kp = a.qkv + (rb + k0 + j) * ld + a.H + hd * dh;
      const float dj = sds[wl][j];
      if (lane < dh) g0 = fmaf(dj, ldf<T>(kp + lane), g0);
      if (lane + 64 < dh) g1 = fmaf(dj, ldf<T>(kp + lane + 64), g1);
    }
  }
  T* gp = a.dqkv + (rb + q) * ld + hd * dh;
  if (lane < dh) stf<T>(gp + lane, g0);
  if (lane + 64 < dh) stf<T>(gp + lane + 64, g1);
}

// dK, dV: one wave per (b,h,key)
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dkv_simple_kernel(SArgs<T> a) {
  __shared__ float sk[4][128];
  __shared__ float sv[4][128];
  __shared__ float sds[4][64];
  __shared__ float spp[4][64];
  const int lane = threadIdx.x & 63, wl = threadIdx.x >> 6;
  const long long wave = (long long)blockIdx.x * 4 + wl;
  if (wave >= (long long)a.B * a.A * a.L) return;
  const int k = (int)(wave % a.L);
  const int hd = (int)((wave / a.L) % a.A);
  const int b = (int)(wave / ((long long)a.L * a.A));
  const int ld = 3 * a.H, dh = a.dh;
  const size_t rb = (size_t)b * a.L;
  const T* kp = a.qkv + (rb + k) * ld + a.H + hd * dh;
  const T* vp = kp + a.H;
  for (int i = lane; i < dh; i += 64) { sk[wl][i] = ldf<T>(kp + i); sv[wl][i] = ldf<T>(vp + i); }
  float gk0 = 0.f, gk1 = 0.f, gv0 = 0.f, gv1 = 0.f;
  const size_t sb = ((size_t)b * a.A + hd) * a.L;
  for (int q0 = 0; q0 < a.L; q0 += 64) {
    const int q = q0 + lane;
    float ds = 0.f, p = 0.f;
    if (q < a.L) {
      const T* qp = a.qkv + (rb + q) * ld + hd * dh;
      const T* dop = a.dctx + (rb + q) * a.H + hd * dh;
      float acc = 0.f, dp = 0.f;
      for (int i = 0; i < dh; ++i) { acc = fmaf(sk[wl][i], ldf<T>(qp + i), acc); dp = fmaf(sv[wl][i], ldf<T>(dop + i), dp); }
      const uint32_t w = a.bits[(rb + q) * a.W + (k >> 5)];
      const float s = acc * a.scale + (((w >> (k & 31)) & 1u) ? 0.f : MASK_ADD);
      p = expf(s - a.lse_in[sb + q]);
      float keepf = 1.0f;
      if (a.dropbits) keepf = attn_keep_bit(a.dropbits, a.NQB, a.NKT, (size_t)b * a.A + hd, q, k) ? a.inv_keep : 0.f;
      ds = p * (keepf * dp - a.delta[sb + q]) * a.scale;
      p *= keepf;
    }
    sds[wl][lane] = ds;
    spp[wl][lane] = p;
    const int qn = min(64, a.L - q0);
    for (int j = 0; j < qn; ++j) {
      const T* qp = a.qkv + (rb + q0 + j) * ld + hd * dh;
      const T* dop = a.dctx + (rb + q0 + j) * a.H + hd * dh;
      const float dj = sds[wl][j], pj = spp[wl][j];
      if (lane < dh) { gk0 = fmaf(dj, ldf<T>(qp + lane), gk0); gv0 = fmaf(pj, ldf<T>(dop + lane), gv0); }
      if (lane + 64 < dh) { gk1 = fmaf(dj, ldf<T>(qp + lane + 64), gk1); gv1 = fmaf(pj, ldf<T>(dop + lane + 64), gv1); }
    }
  }
  T* gk = a.dqkv + (rb + k) * ld + a.H + hd * dh;
  T* gv = gk + a.H;
  if (lane < dh) { stf<T>(gk + lane, gk0); stf<T>(gv + lane, gv0); }
  if (lane + 64 < dh) { stf<T>(gk + lane + 64, gk1); stf<T>(gv + lane + 64, gv1); }
}

template <typename T>
static SArgs<T> simple_args(const void* qkv, const uint32_t* bits, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits) {
  SArgs<T> s{};
  attn_fill_common(s, B, L, A, dh, p_drop, dropbits);
  s.qkv = (const T*)qkv; s.bits = bits; s.dh = dh;
  return s;
}

int mv_attn_simple_fwd(int dtype, const void* qkv, const uint32_t* bits, void* ctx, float* lse, int B, int L, int A, int dh, float p_drop,
                       const uint32_t* dropbits, hipStream_t stream) {
  return mv_with_type(dtype, [&](auto t) -> int {
    typedef MV_T(t) T;
    SArgs<T> s = simple_args<T>(qkv, bits, B, L, A, dh, p_drop, dropbits);
    s.out = (T*)ctx; s.lse = lse;
    const long long waves = (long long)B * A * L;
    hipLaunchKernelGGL(attn_fwd_simple_kernel<T>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, s);
    return (int)hipGetLastError();
  });
}

int mv_attn_simple_bwd(int dtype, const void* qkv, const void* ctx, const void* dctx, const float* lse, const uint32_t* bits, void* dqkv,
                       float* delta, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits, hipStream_t stream) {
  return mv_with_type(dtype, [&](auto t) -> int {
    typedef MV_T(t) T;
    SArgs<T> s = simple_args<T>(qkv, bits, B, L, A, dh, p_drop, dropbits);
    s.ctx = (const T*)ctx; s.dctx = (const T*)dctx; s.dqkv = (T*)dqkv;
    s.lse_in = lse; s.delta = delta;
    const long long waves = (long long)B * A * L;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    hipLaunchKernelGGL(attn_delta_kernel<T>, dim3(blocks), dim3(256), 0, stream, s.ctx, s.dctx, delta, B, L, A, s.H, dh);
    MV_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_bwd_dq_simple_kernel<T>, dim3(blocks), dim3(256), 0, stream, s);
    MV_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_bwd_dkv_simple_kernel<T>, dim3(blocks), dim3(256), 0, stream, s);
    return (int)hipGetLastError();
  });
}
