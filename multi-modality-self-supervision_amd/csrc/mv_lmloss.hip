// Report-generation fine-tuning (DESIGN.md "8e. Report fine-tuning"): the masked-LM objective of the reference's
// BertForPreTrainingLossMask(tasks='report_generation') -- label-smoothed KL (or plain CE), per-entry weights, several entries per
// logit row, drop-worst sample selection, normalisation by the kept weight sum -- over the DISTINCT consumed rows.
//
//   mv_lm_loss_fwd     one block per row: online log-sum-exp, column sum, argmax in one pass; the loss of every entry of the row
//   mv_lm_loss_select  one block: per-sample sums in entry order, the k smallest, the scalar loss and 1 / denominator (no f32 atomics:
//                      the same input gives the same bits)
//   mv_lm_loss_bwd     one block per row: g * S / denominator * sum over the row's kept entries of w (Q softmax - q)
//
// Rows are walked with 16-byte loads when the leading dimension and the base allow it (the MLM head's padded [U, Vp] buffers do).
#include "mv_dispatch.h"

namespace {

struct LmRow {          // what one pass over a row yields (the same value in every thread after lm_row_reduce)
  float m;              // max
  double s;             // sum exp(z - m)
  double zs;            // sum of z over columns 1 .. V-1
  int am;               // first argmax
};

__device__ __forceinline__ void lm_take(LmRow& r, float x, int c) {
  if (x > r.m) {                                          // (also the first finite value: exp(-inf) = 0 and s = 0)
    r.s = r.s * (double)expf(r.m - x) + 1.0;
    r.m = x;
    r.am = c;
  } else if (x > -INFINITY) {
    r.s += (double)expf(x - r.m);
  }
  if (c >= 1) r.zs += (double)x;
}

__device__ __forceinline__ void lm_merge(LmRow& r, float om, double os, double oz, int oa) {
  if (om > r.m || (om == r.m && oa < r.am)) r.am = oa;
  const float nm = fmaxf(r.m, om);
  const double a = r.m > -INFINITY ? r.s * (double)expf(r.m - nm) : 0.0;
  const double b = om > -INFINITY ? os * (double)expf(om - nm) : 0.0;
  r.s = a + b;
  r.m = nm;
  r.zs += oz;
}

template <bool VEC>
__device__ __forceinline__ LmRow lm_row_pass(const float* __restrict__ zr, int V) {
  LmRow r{-INFINITY, 0.0, 0.0, 0x7fffffff};
  const int tid = threadIdx.x;
  if (VEC) {
    for (int c = tid * 4; c < V; c += 1024) {
      const f32x4 x = ld4<float>(zr + c);                 // (c + 3 < ld: ld is a multiple of 4 and >= V)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < V) lm_take(r, x[e], c + e);
    }
  } else {
    for (int c = tid; c < V; c += 256) lm_take(r, zr[c], c);
  }
  return r;
}

// wave shuffle, then the four waves' partials in wave order: every thread ends with the same bits
__device__ __forceinline__ void lm_row_reduce(LmRow& r, float* s_m, double* s_s, double* s_z, int* s_a) {
  const int lane = threadIdx.x & 63, wl = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(r.m, o, 64);
    const double os = __shfl_xor(r.s, o, 64), oz = __shfl_xor(r.zs, o, 64);
    const int oa = __shfl_xor(r.am, o, 64);
    LmRow mine = r;
    // both partners must form the same sum: the lower lane's value is always the left operand
    if (lane & o) { LmRow t{om, os, oz, oa}; lm_merge(t, mine.m, mine.s, mine.zs, mine.am); r = t; }
    else lm_merge(r, om, os, oz, oa);
  }
  if (lane == 0) { s_m[wl] = r.m; s_s[wl] = r.s; s_z[wl] = r.zs; s_a[wl] = r.am; }
  __syncthreads();
  r = LmRow{s_m[0], s_s[0], s_z[0], s_a[0]};
  for (int w = 1; w < 4; ++w) lm_merge(r, s_m[w], s_s[w], s_z[w], s_a[w]);
}

// ------------------------------------------------------------------------------------------------ forward
// conf = 1 - label_smoothing; sval = label_smoothing / (V - 2) rounded to f32 as the reference's torch.full does (loss.py:28-29).  The
// few operations per entry run in double: the closed form cancels terms of size (V - 2) * lse.
template <bool VEC>
__global__ __launch_bounds__(256) void lm_fwd_kernel(const float* __restrict__ logits, int ld, int V, const int32_t* __restrict__ row_ptr,
                                                     const int32_t* __restrict__ labels, double conf, float sval, int smooth,
                                                     float* __restrict__ entry_loss, int32_t* __restrict__ entry_hit,
                                                     float* __restrict__ row_stat) {
  __shared__ float s_m[4];
  __shared__ double s_s[4], s_z[4];
  __shared__ int s_a[4];
  const int u = blockIdx.x, tid = threadIdx.x;
  const float* zr = logits + (size_t)u * ld;
  LmRow r = lm_row_pass<VEC>(zr, V);
  lm_row_reduce(r, s_m, s_s, s_z, s_a);
  const float sf = (float)r.s;
  if (tid == 0) { row_stat[2 * (size_t)u] = r.m; row_stat[2 * (size_t)u + 1] = sf; }
  const double lse = (double)r.m + log((double)sf);       // (the backward forms softmax from the same rounded pair)
  const int e0 = row_ptr[u], e1 = row_ptr[u + 1];
  for (int e = e0 + tid; e < e1; e += 256) {
    const int t = labels[e];
    if ((unsigned)t >= (unsigned)V) {                     // outside the contract (the host plan refuses it): nothing is read
      entry_loss[e] = NAN;
      if (entry_hit) entry_hit[e] = 0;
      continue;
    }
    const double zt = (double)zr[t];
    double loss;
    if (!smooth) {
      loss = lse - zt;                                    // CrossEntropyLoss(reduction='none'): label 0 counts (model.py:1050)
    } else if (t == 0) {
      loss = 0.0;                                         // ignore_index = 0: the whole target row is zero (loss.py:46)
    } else {
      const double c = conf, s = (double)sval, n = (double)(V - 2);
      loss = (c > 0.0 ? c * log(c) : 0.0) + n * s * log(s) - c * (zt - lse) - s * ((r.zs - zt) - n * lse);
    }
    entry_loss[e] = (float)loss;
    if (entry_hit) entry_hit[e] = (r.am == t) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ selection
// loss_mask_and_normalize (model.py:998-1005) for the per-sample sums of w * loss: the k smallest are kept (ties to the lower sample).
__global__ __launch_bounds__(256) void lm_select_kernel(const float* __restrict__ entry_loss, const float* __restrict__ weights,
                                                        const int32_t* __restrict__ sample, const int32_t* __restrict__ entry_hit, int n,
                                                        int B, int k, int32_t* __restrict__ keep, float* __restrict__ stats,
                                                        float* __restrict__ inv_denom) {
  extern __shared__ double lm_sh[];
  double* L = lm_sh;
  double* W = lm_sh + B;
  int* Hh = (int*)(lm_sh + 2 * (size_t)B);
  int* K = Hh + B;
  const int tid = threadIdx.x;
  for (int b = tid; b < B; b += 256) {
    double l = 0.0, w = 0.0;
    int h = 0;
    for (int e = 0; e < n; ++e) {                         // entry order: a fixed summation order per sample
      if (sample[e] != b) continue;
      const float wt = weights[e];
      l += (double)wt * (double)entry_loss[e];
      w += (double)wt;
      if (wt > 0.f && entry_hit && entry_hit[e]) ++h;
    }
    L[b] = l; W[b] = w; Hh[b] = h;
  }
  __syncthreads();
  for (int b = tid; b < B; b += 256) {
    const double lb = L[b];
    int rank = 0;
    for (int j = 0; j < B; ++j) rank += (L[j] < lb || (L[j] == lb && j < b)) ? 1 : 0;
    const int kp = rank < k ? 1 : 0;
    K[b] = kp;
    keep[b] = kp;
  }
  __syncthreads();
  if (tid != 0) return;
  double ls = 0.0, ws = 0.0;
  int cnt = 0, hits = 0;
  for (int b = 0; b < B; ++b)
    if (K[b]) { ls += L[b]; ws += W[b]; ++cnt; hits += Hh[b]; }
  const double den = ws + 1e-5;
  stats[0] = (float)(ls / den);
  stats[1] = (float)ws;
  stats[2] = (float)cnt;
  stats[3] = (float)hits;
  *inv_denom = (float)(1.0 / den);
}

// ------------------------------------------------------------------------------------------------ backward
template <typename TD, bool VEC>
__global__ __launch_bounds__(256) void lm_bwd_kernel(const float* __restrict__ logits, int ld, int V, const int32_t* __restrict__ row_ptr,
                                                     const int32_t* __restrict__ labels, const float* __restrict__ weights,
                                                     const int32_t* __restrict__ sample, float conf, float sval, float qsum, int smooth,
                                                     const float* __restrict__ row_stat, const int32_t* __restrict__ keep,
                                                     const float* __restrict__ inv_denom, const float* __restrict__ grad_dev,
                                                     const float* __restrict__ ls_dev, TD* __restrict__ dlogits, int ldd) {
  const int u = blockIdx.x, tid = threadIdx.x;
  const int e0 = row_ptr[u], e1 = row_ptr[u + 1];
  TD* dr = dlogits + (size_t)u * ldd;
  // the row's kept mass (every thread walks the same few entries in the same order)
  float amass = 0.f, wsm = 0.f;
  bool any = false;
  for (int e = e0; e < e1; ++e) {
    const float cf = keep[sample[e]] ? weights[e] : 0.f;
    if (!(cf > 0.f) || (smooth && labels[e] == 0)) continue;
    amass += cf * qsum;
    wsm += cf;
    any = true;
  }
  if (!any) {                                             // dropped, zero-weight or ignored throughout: no logit is read
    if (VEC) for (int c = tid * 4; c < ldd; c += 1024) st4<TD>(dr + c, (f32x4){0.f, 0.f, 0.f, 0.f});
    else for (int c = tid; c < ldd; c += 256) stf<TD>(dr + c, 0.f);
    return;
  }
  const float* zr = logits + (size_t)u * ld;
  const float G = *grad_dev * (ls_dev ? *ls_dev : 1.0f) * *inv_denom;
  const float M = row_stat[2 * (size_t)u], inv_s = 1.0f / row_stat[2 * (size_t)u + 1];
  const float base = smooth ? sval * wsm : 0.f;           // every column >= 1 carries the smoothing value ...
  const float hot = smooth ? conf - sval : 1.0f;          // ... and the label's column the confidence instead
  if (VEC) {
    for (int c = tid * 4; c < ldd; c += 1024) {
      f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c < V) {
        const f32x4 x = ld4<float>(zr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < V) o[e] = amass * (expf(x[e] - M) * inv_s) - ((c + e) >= 1 ? base : 0.f);
        for (int e = e0; e < e1; ++e) {
          const int t = labels[e];
          if (t < c || t >= c + 4 || t >= V || (smooth && t == 0)) continue;
          const float cf = keep[sample[e]] ? weights[e] : 0.f;
          if (cf > 0.f) o[t - c] -= cf * hot;
        }
        o *= G;
      }
      st4<TD>(dr + c, o);
    }
  } else {
    for (int c = tid; c < ldd; c += 256) {
      float o = 0.f;
      if (c < V) {
        o = amass * (expf(zr[c] - M) * inv_s) - (c >= 1 ? base : 0.f);
        for (int e = e0; e < e1; ++e) {
          if (labels[e] != c || (smooth && c == 0)) continue;
          const float cf = keep[sample[e]] ? weights[e] : 0.f;
          if (cf > 0.f) o -= cf * hot;
        }
        o *= G;
      }
      stf<TD>(dr + c, o);
    }
  }
}

struct LmConst { double conf; float sval, qsum; int smooth; };
inline LmConst lm_const(double label_smoothing, int V) {
  LmConst k;
  k.smooth = label_smoothing > 0.0 ? 1 : 0;
  k.conf = 1.0 - label_smoothing;
  k.sval = k.smooth ? (float)(label_smoothing / (double)(V - 2)) : 0.f;
  k.qsum = k.smooth ? (float)(k.conf + (double)(V - 2) * (double)k.sval) : 1.0f;   // the mass of a smoothed target row
  return k;
}
inline int lm_check(const float* logits, int ld, int U, int V, const int32_t* row_ptr, const int32_t* labels, int n_entries,
                    double label_smoothing) {
  if (U < 0 || n_entries < 0 || V <= 0 || ld < V) return MV_E_ARG;
  if (!(label_smoothing >= 0.0 && label_smoothing <= 1.0)) return MV_E_ARG;
  if (label_smoothing > 0.0 && V < 3) return MV_E_ARG;
  if (U > 0 && (!logits || !row_ptr)) return MV_E_ARG;
  if (n_entries > 0 && !labels) return MV_E_ARG;
  return MV_OK;
}

}  // namespace

extern "C" int mv_lm_loss_fwd(const float* logits, int ld, int U, int V, const int32_t* row_ptr, const int32_t* labels, int n_entries,
                              double label_smoothing, float* entry_loss, int32_t* entry_hit, float* row_stat, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = lm_check(logits, ld, U, V, row_ptr, labels, n_entries, label_smoothing);
  if (rc) return rc;
  if (U > 0 && !row_stat) return MV_E_ARG;
  if (n_entries > 0 && !entry_loss) return MV_E_ARG;
  if (U == 0) return MV_OK;
  const LmConst k = lm_const(label_smoothing, V);
  const bool vec = (ld & 3) == 0 && (((uintptr_t)logits) & 15) == 0;
  const dim3 grid(U), block(256);
  if (vec) hipLaunchKernelGGL(lm_fwd_kernel<true>, grid, block, 0, stream, logits, ld, V, row_ptr, labels, k.conf, k.sval, k.smooth, entry_loss, entry_hit, row_stat);
  else hipLaunchKernelGGL(lm_fwd_kernel<false>, grid, block, 0, stream, logits, ld, V, row_ptr, labels, k.conf, k.sval, k.smooth, entry_loss, entry_hit, row_stat);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_lm_loss_select(const float* entry_loss, const float* weights, const int32_t* sample, const int32_t* entry_hit,
                                 int n_entries, int B, int k, int32_t* keep, float* stats, float* inv_denom, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_entries < 0 || B <= 0 || k < 0 || !keep || !stats || !inv_denom) return MV_E_ARG;
  if (n_entries > 0 && (!entry_loss || !weights || !sample)) return MV_E_ARG;
  if (B > 2048) return MV_E_SHAPE;                        // the per-sample sums live in LDS (24 bytes per sample)
  const size_t lds = (size_t)B * (2 * sizeof(double) + 2 * sizeof(int));
  hipLaunchKernelGGL(lm_select_kernel, dim3(1), dim3(256), lds, stream, entry_loss, weights, sample, entry_hit, n_entries, B, k, keep, stats, inv_denom);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

extern "C" int mv_lm_loss_bwd(const float* logits, int ld, int U, int V, const int32_t* row_ptr, const int32_t* labels,
                              const float* weights, const int32_t* sample, int n_entries, double label_smoothing,
                              const float* row_stat, const int32_t* keep, const float* inv_denom, const float* grad_dev,
                              const float* loss_scale_dev, void* dlogits, int d_dtype, int ldd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = lm_check(logits, ld, U, V, row_ptr, labels, n_entries, label_smoothing);
  if (rc) return rc;
  if (!keep || !inv_denom || !grad_dev) return MV_E_ARG;
  if (U > 0 && (!row_stat || !dlogits)) return MV_E_ARG;
  if (n_entries > 0 && (!weights || !sample)) return MV_E_ARG;
  if (!mv_dtype_ok(d_dtype)) return MV_E_DTYPE;
  if (ldd < V) return MV_E_SHAPE;
  if (U == 0) return MV_OK;
  const LmConst k = lm_const(label_smoothing, V);
  const uintptr_t dal = (uintptr_t)(4 * mv_dtype_size(d_dtype) - 1);
  const bool vec = (ld & 3) == 0 && (ldd & 3) == 0 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)dlogits) & dal) == 0;
  const dim3 grid(U), block(256);
  return mv_with_type(d_dtype, [&](auto t) -> int {
    typedef MV_T(t) TD;
    auto launch = [&](auto kernel) -> int {
      hipLaunchKernelGGL(kernel, grid, block, 0, stream, logits, ld, V, row_ptr, labels, weights, sample, (float)k.conf, k.sval, k.qsum, k.smooth,
                         row_stat, keep, inv_denom, grad_dev, loss_scale_dev, (TD*)dlogits, ldd);
      return (int)hipGetLastError();
    };
    return vec ? launch(lm_bwd_kernel<TD, true>) : launch(lm_bwd_kernel<TD, false>);
  });
}
