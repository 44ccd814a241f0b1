// The fine-tuning optimizer of the reference's downstream programs and the loss of its diagnosis classifier:
//
//   mv_tensor_sqnorms  sum of squares of every tensor of a flat f32 buffer (BertAdam clips each tensor by its OWN gradient norm)
//   mv_bertadam_step   BertAdam (pytorch_pretrained_bert/optimization.py:112-182) over the flat buffer in one launch
//   mv_bce_multilabel  BCEWithLogitsLoss(pos_weight) over multi-hot targets, its gradient, probabilities and tp / fp / fn counters
//
// The first two are driven by two device tables that the host builds once per model:
//   tensors int64 [T, 4] = {offset, count, first_chunk, flags}   flags: bit 0 = weight decay applies, bit 1 = active
//   chunks  int32 [NC]   = tensor id of every MV_OPTIM_CHUNK-element chunk; a tensor of `count` elements owns
//                          ceil(count / MV_OPTIM_CHUNK) consecutive chunks starting at first_chunk
// Tensor sizes span 2 elements to 23 M, so a block works on one equal-sized chunk rather than on one tensor.  Offsets are multiples
// of 64 elements (engine._align), so a chunk never holds elements of two tensors and every 16-byte access is aligned.
#include "mv_dispatch.h"

#define MV_LS_SKIP 3          // device state of the dynamic loss scale (mv_rowops.hip): [3] skip flag, [4] optimizer steps applied
#define MV_LS_T 4
#define CH MV_OPTIM_CHUNK
static_assert(CH % 1024 == 0, "a chunk is a whole number of 256-thread x 4-element passes");

// ------------------------------------------------------------------------------------------------ mv_tensor_sqnorms
// Pass 1: block = chunk; a thread sums its CH / 256 elements in index order, the wave by xor-shuffles, the four waves in wave order.
// Pass 2: wave = tensor; lane l sums partials l, l + 64, ... in order, then the same shuffles.  No atomics anywhere: the order of
// every addition is fixed by the tables, so two runs over the same data give the same bits.
__global__ __launch_bounds__(256) void sq_chunk_kernel(const float* __restrict__ x, size_t n, const long long* __restrict__ tensors,
                                                       const int32_t* __restrict__ chunks, float* __restrict__ partials) {
  __shared__ float s_w[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int t = chunks[c];
  const long long* tt = tensors + 4 * (size_t)t;
  const long long k = c - tt[2];
  float s = 0.f;
  if ((tt[3] & 2) && k >= 0) {                            // an inactive tensor's norm is never read
    const long long left = tt[1] - k * CH;
    const int len = (int)(left < CH ? left : CH);
    const size_t base = (size_t)tt[0] + (size_t)k * CH;
#pragma unroll
    for (int pass = 0; pass < CH / 1024; ++pass) {
      const int j = pass * 1024 + tid * 4;
      if (j < len && base + j + 4 <= n) {
        const f32x4 v = *(const f32x4*)(x + base + j);     // the last vector of a tensor may reach into the alignment gap: masked
#pragma unroll
        for (int e = 0; e < 4; ++e) s += (j + e < len) ? v[e] * v[e] : 0.f;
      }
    }
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) s_w[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partials[c] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(64) void sq_tensor_kernel(const long long* __restrict__ tensors, const float* __restrict__ partials, int NC,
                                                       float* __restrict__ out) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const long long* tt = tensors + 4 * (size_t)t;
  const long long first = tt[2], nch = (tt[1] + CH - 1) / CH;
  float s = 0.f;
  if (tt[3] & 2)
    for (long long i = lane; i < nch && first + i < NC; i += 64) s += partials[first + i];
  s = wave_sum(s);
  if (lane == 0) out[t] = s;
}

extern "C" int mv_tensor_sqnorms(const float* x, size_t n, const int64_t* tensors, int T, const int32_t* chunks, int NC, float* partials,
                                 float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !tensors || !chunks || !partials || !out || n == 0 || T <= 0 || NC <= 0) return MV_E_ARG;
  if ((((uintptr_t)x) & 15) || (n & 3)) return MV_E_SHAPE;
  hipLaunchKernelGGL(sq_chunk_kernel, dim3(NC), dim3(256), 0, stream, x, n, (const long long*)tensors, chunks, partials);
  MV_CHECK_LAUNCH();
  hipLaunchKernelGGL(sq_tensor_kernel, dim3(T), dim3(64), 0, stream, (const long long*)tensors, partials, NC, out);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

// ------------------------------------------------------------------------------------------------ mv_bertadam_step
// lr * schedule(step / t_total, warmup) in double like the reference's Python floats (optimization.py:33-48,165-170), rounded to f32
// once: the reference multiplies an f32 tensor by that Python float.
__device__ __forceinline__ float bertadam_lr(double lr, int step, int t_total, double warmup, int schedule) {
  if (t_total == -1) return (float)lr;
  const double x = (double)step / (double)t_total;
  double f;
  if (x < warmup) f = x / warmup;
  else if (schedule == MV_SCHED_WARMUP_CONSTANT) f = 1.0;
  else if (schedule == MV_SCHED_WARMUP_COSINE) f = 0.5 * (1.0 + cos(3.14159265358979323846 * x));
  else { f = (x - 1.0) / (warmup - 1.0); if (!(f > 0.0)) f = 0.0; }
  return (float)(lr * f);
}

// (omb1 = 1 - b1 and omb2 = 1 - b2 are formed in double on the host and rounded once, like the reference's Python floats)
__device__ __forceinline__ void bertadam_elem(float& p, float g, float& m, float& v, float clip, float b1, float omb1, float b2, float omb2,
                                              float eps, float wd, float lr_t) {
  g *= clip;
  m = b1 * m + omb1 * g;
  v = b2 * v + omb2 * g * g;
  float u = m / (sqrtf(v) + eps);
  if (wd > 0.f) u += wd * p;
  p -= lr_t * u;
}

// Block = chunk, as pass 1 above.  Per element: clip factor of its tensor, moments, decoupled decay, p -= lr_t * u, and the 16-bit
// copies the MFMA kernels read.  Elements outside every tensor (alignment gaps) and inactive tensors are neither read nor written.
__global__ __launch_bounds__(256) void bertadam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, bf16_t* __restrict__ shadow, f16_t* __restrict__ shadow16,
                                                       size_t n, const long long* __restrict__ tensors, const int32_t* __restrict__ chunks,
                                                       const float* __restrict__ sqnorms, double lr, float b1, float omb1, float b2, float omb2, float eps,
                                                       float weight_decay, float max_grad_norm, int step, int t_total, double warmup,
                                                       int schedule, const float* __restrict__ state) {
  if (state) {
    if (state[MV_LS_SKIP] != 0.f) return;                 // overflowed step: nothing changes, the schedule does not advance
    step = (int)state[MV_LS_T] - 1;                       // mv_scaler_update has counted this step already; the rule reads `step` BEFORE
    if (step < 0) step = 0;                               // a freshly reset state (no update counted yet): the first step, never lr < 0
  }
  const int c = blockIdx.x, tid = threadIdx.x;
  const int t = chunks[c];
  const long long* tt = tensors + 4 * (size_t)t;
  const long long flags = tt[3], k = c - tt[2];
  if (!(flags & 2) || k < 0) return;
  const long long left = tt[1] - k * CH;
  const int len = (int)(left < CH ? left : CH);
  const size_t base = (size_t)tt[0] + (size_t)k * CH;
  const float lr_t = bertadam_lr(lr, step, t_total, warmup, schedule);
  const float wd = (flags & 1) ? weight_decay : 0.f;
  // clip_grad_norm_ on ONE tensor: g *= min(1, max_norm / (||g|| + 1e-6)), f32 like the reference's tensors
  const float clip = (max_grad_norm > 0.f && sqnorms) ? fminf(max_grad_norm / (sqrtf(sqnorms[t]) + 1e-6f), 1.0f) : 1.0f;
#pragma unroll
  for (int pass = 0; pass < CH / 1024; ++pass) {
    const int j = pass * 1024 + tid * 4;
    if (j >= len || base + j + 4 > n) continue;
    const size_t i = base + j;
    if (j + 4 <= len) {
      f32x4 pp = *(const f32x4*)(p + i), gg = *(const f32x4*)(g + i), mm = *(const f32x4*)(m + i), vv = *(const f32x4*)(v + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        bertadam_elem(pe, gg[e], me, ve, clip, b1, omb1, b2, omb2, eps, wd, lr_t);
        pp[e] = pe; mm[e] = me; vv[e] = ve;
      }
      *(f32x4*)(p + i) = pp; *(f32x4*)(m + i) = mm; *(f32x4*)(v + i) = vv;
      if (shadow) st4<bf16_t>(shadow + i, pp);
      if (shadow16) st4<f16_t>(shadow16 + i, pp);
    } else {
      for (int e = 0; j + e < len; ++e) {                 // the last 1-3 elements of a tensor: the gap behind them stays untouched
        float pe = p[i + e], me = m[i + e], ve = v[i + e];
        bertadam_elem(pe, g[i + e], me, ve, clip, b1, omb1, b2, omb2, eps, wd, lr_t);
        p[i + e] = pe; m[i + e] = me; v[i + e] = ve;
        if (shadow) shadow[i + e] = (bf16_t)pe;
        if (shadow16) shadow16[i + e] = (f16_t)pe;
      }
    }
  }
}

extern "C" int mv_bertadam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, void* shadow_f16, size_t n,
                                const int64_t* tensors, int T, const int32_t* chunks, int NC, const float* sqnorms, double lr, double b1,
                                double b2, float eps, float weight_decay, float max_grad_norm, int step, int t_total, double warmup,
                                int schedule, const float* scaler_state, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!p || !g || !m || !v || !tensors || !chunks || n == 0 || T <= 0 || NC <= 0) return MV_E_ARG;
  if (max_grad_norm > 0.f && !sqnorms) return MV_E_ARG;
  if ((step < 0 && !scaler_state) || (t_total != -1 && t_total <= 0)) return MV_E_ARG;
  if (schedule != MV_SCHED_WARMUP_LINEAR && schedule != MV_SCHED_WARMUP_CONSTANT && schedule != MV_SCHED_WARMUP_COSINE) return MV_E_ARG;
  if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) || (n & 3)) return MV_E_SHAPE;
  if ((shadow_bf16 && (((uintptr_t)shadow_bf16) & 7)) || (shadow_f16 && (((uintptr_t)shadow_f16) & 7))) return MV_E_SHAPE;
  hipLaunchKernelGGL(bertadam_kernel, dim3(NC), dim3(256), 0, stream, p, g, m, v, (bf16_t*)shadow_bf16, (f16_t*)shadow_f16, n,
                     (const long long*)tensors, chunks, sqnorms, lr, (float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), eps, weight_decay, max_grad_norm, step, t_total, warmup,
                     schedule, scaler_state);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

// ------------------------------------------------------------------------------------------------ mv_bce_multilabel
// Wave = one row (C is the number of findings: 14 for CheXpert-style labels).  Per column the stable element loss
//   (1 - y) z + (1 + (w - 1) y) (max(-z, 0) + log1p(exp(-|z|)))          (torch's binary_cross_entropy_with_logits with pos_weight)
// its gradient (sigmoid(z) (w y + 1 - y) - w y) g S, the probability sigmoid(z) and the counters at threshold 0.5 (z > 0).
template <typename TD>
__global__ __launch_bounds__(64) void bce_ml_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ target,
                                                    const float* __restrict__ pos_weight, int C, float* __restrict__ loss,
                                                    TD* __restrict__ dgrad, int ldd, const float* __restrict__ gs_dev, float gs_host,
                                                    const float* __restrict__ ls_dev, float* __restrict__ probs,
                                                    float* __restrict__ counters) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* zr = logits + (size_t)row * ld;
  const float* yr = target ? target + (size_t)row * C : nullptr;
  TD* dr = dgrad ? dgrad + (size_t)row * ldd : nullptr;
  const float gs = dr ? (gs_dev ? *gs_dev : gs_host) * (ls_dev ? *ls_dev : 1.0f) : 0.f;
  float acc = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float z = zr[c];
    const float e = expf(-fabsf(z));
    const float sg = z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);      // sigmoid(z) without overflow
    if (probs) probs[(size_t)row * C + c] = sg;
    if (yr) {
      const float y = yr[c], w = pos_weight ? pos_weight[c] : 1.0f;
      acc += (1.0f - y) * z + (1.0f + (w - 1.0f) * y) * (fmaxf(-z, 0.f) + log1pf(e));
      if (dr) stf<TD>(dr + c, (sg * (w * y + 1.0f - y) - w * y) * gs);
      if (counters) {
        const bool pos = y > 0.5f, pred = z > 0.f;
        if (pred && pos) atomicAdd(counters + c, 1.0f);                  // integer-valued f32 counts: exact, order-free below 2^24
        else if (pred) atomicAdd(counters + C + c, 1.0f);
        else if (pos) atomicAdd(counters + 2 * C + c, 1.0f);
      }
    }
  }
  if (dr) for (int c = C + lane; c < ldd; c += 64) stf<TD>(dr + c, 0.f);   // padding columns: the next GEMM contracts over them
  if (loss && yr) {
    acc = wave_sum(acc);
    if (lane == 0) atomicAdd(loss, acc);
  }
}

extern "C" int mv_bce_multilabel(const float* logits, int ld, const float* target, const float* pos_weight, int R, int C, float* loss,
                                 void* dgrad, int d_dtype, int ldd, const float* grad_scale_dev, float grad_scale_host,
                                 const float* loss_scale_dev, float* probs, float* counters, void* stream_) {
  typedef mv_types<float, bf16_t, f16_t> Accept;      // of dgrad; without dgrad, d_dtype is not looked at (the float instantiation runs)
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || R <= 0 || C <= 0 || ld < C) return MV_E_ARG;
  if ((loss || dgrad || counters) && !target) return MV_E_ARG;
  if (dgrad && ldd < C) return MV_E_SHAPE;
  const dim3 grid(R), block(64);
  return mv_with_type(dgrad ? d_dtype : MV_F32, Accept{}, [&](auto t) -> int {
    typedef MV_T(t) TD;
    hipLaunchKernelGGL((bce_ml_kernel<TD>), grid, block, 0, stream, logits, ld, target, pos_weight, C, loss, (TD*)dgrad, ldd, grad_scale_dev,
                       grad_scale_host, loss_scale_dev, probs, counters);
    return (int)hipGetLastError();
  });
}
