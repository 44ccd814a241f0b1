// VQA fine-tuning / answer prediction (DESIGN.md "8b. VQA"): the kernels of the answer classifier's loss and of the inference
// embedding that the pretraining and generation kernels do not cover.  The classifier's two products run on mv_gemm_rows
// (16-bit) / mv_gemm (f32); its ReLU backward is mv_dact mode 2.
//
//   mv_bce_fwd_bwd  BCEWithLogits over soft targets (sum), its gradient, the training / inference argmax and the VQA score split
//   mv_rows_mul     out[i] = a[rows_a[i]] * b[rows_b[i]]   (the [CLS] (.) [SEP] inference embedding from the compact hidden state)
#include "mv_dispatch.h"

// ------------------------------------------------------------------------------------------------ mv_bce_fwd_bwd
// Block = one row, 256 threads walk its columns (A = 458: two per thread).  Per column: the stable element loss
// max(z,0) - z*y + log1p(exp(-|z|)) and the gradient (sigmoid(z) - y) * gs; per row: the two argmaxes (ties to the lower column,
// as torch.max), then one thread adds the row's loss, its score y[argmax] and the split counters with six f32 atomics.
template <typename TD>
__global__ __launch_bounds__(256) void bce_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ target,
                                                  const int32_t* __restrict__ ans_type, int A, float* __restrict__ stats,
                                                  TD* __restrict__ dgrad, int ldd, const float* __restrict__ gs_dev, float gs_host,
                                                  const float* __restrict__ ls_dev, int64_t* __restrict__ arg_train,
                                                  int64_t* __restrict__ arg_infer) {
  __shared__ float s_loss[4], s_mt[4], s_mi[4];
  __shared__ int s_at[4], s_ai[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wl = tid >> 6;
  const float* zr = logits + (size_t)row * ld;
  const float* yr = target ? target + (size_t)row * A : nullptr;
  TD* dr = dgrad ? dgrad + (size_t)row * ldd : nullptr;
  const float gs = dr ? (gs_dev ? *gs_dev : gs_host) * (ls_dev ? *ls_dev : 1.0f) : 0.f;   // x loss scale (16-bit gradients)
  float loss = 0.f, mt = -INFINITY, mi = -INFINITY;
  int at = 0x7fffffff, ai = 0x7fffffff;
  for (int c = tid; c < A; c += 256) {
    const float z = zr[c];
    if (z > mt) { mt = z; at = c; }                       // columns grow per thread: the first maximum is kept
    if (c >= 1 && z > mi) { mi = z; ai = c; }
    if (yr) {
      const float y = yr[c];
      const float e = expf(-fabsf(z));
      loss += fmaxf(z, 0.f) - z * y + log1pf(e);
      if (dr) {
        const float sg = z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);     // sigmoid(z) without overflow
        stf<TD>(dr + c, (sg - y) * gs);
      }
    }
  }
  if (dr) for (int c = A + tid; c < ldd; c += 256) stf<TD>(dr + c, 0.f);   // padding columns: the next GEMM contracts over them
  loss = wave_sum(loss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mt, o, 64), oi = __shfl_xor(mi, o, 64);
    const int oa = __shfl_xor(at, o, 64), ob = __shfl_xor(ai, o, 64);
    if (om > mt || (om == mt && oa < at)) { mt = om; at = oa; }
    if (oi > mi || (oi == mi && ob < ai)) { mi = oi; ai = ob; }
  }
  if (lane == 0) { s_loss[wl] = loss; s_mt[wl] = mt; s_at[wl] = at; s_mi[wl] = mi; s_ai[wl] = ai; }
  __syncthreads();
  if (tid != 0) return;
  loss = s_loss[0];
  mt = s_mt[0]; at = s_at[0]; mi = s_mi[0]; ai = s_ai[0];
  for (int w = 1; w < 4; ++w) {
    loss += s_loss[w];
    if (s_mt[w] > mt || (s_mt[w] == mt && s_at[w] < at)) { mt = s_mt[w]; at = s_at[w]; }
    if (s_mi[w] > mi || (s_mi[w] == mi && s_ai[w] < ai)) { mi = s_mi[w]; ai = s_ai[w]; }
  }
  if (at >= A) at = 0;                                    // a row of NaN logits: torch.max would return the NaN's index; 0 is in range
  if (ai >= A) ai = A > 1 ? 1 : 0;
  if (arg_train) arg_train[row] = at;
  if (arg_infer) arg_infer[row] = ai;
  if (stats && yr) {
    const float score = yr[at];                           // one_hot(argmax) . target
    atomicAdd(stats + 0, score);
    atomicAdd(stats + 1, loss);
    const int ty = ans_type ? ans_type[row] : -1;
    if (ty == 0) { atomicAdd(stats + 2, score); atomicAdd(stats + 3, 1.0f); }
    else if (ty == 1) { atomicAdd(stats + 4, score); atomicAdd(stats + 5, 1.0f); }
  }
}

extern "C" int mv_bce_fwd_bwd(const float* logits, int ld, const float* target, const int32_t* ans_type, int R, int A, float* stats,
                              void* dgrad, int d_dtype, int ldd, const float* grad_scale_dev, float grad_scale_host,
                              const float* loss_scale_dev, int64_t* arg_train, int64_t* arg_infer, void* stream_) {
  typedef mv_types<float, bf16_t, f16_t> Accept;      // of dgrad; without dgrad, d_dtype is not looked at (the float instantiation runs)
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || R <= 0 || A <= 0 || ld < A) return MV_E_ARG;
  if ((stats || dgrad) && !target) return MV_E_ARG;
  if (dgrad && ldd < A) return MV_E_SHAPE;
  const dim3 grid(R), block(256);
  return mv_with_type(dgrad ? d_dtype : MV_F32, Accept{}, [&](auto t) -> int {
    typedef MV_T(t) TD;
    hipLaunchKernelGGL((bce_kernel<TD>), grid, block, 0, stream, logits, ld, target, ans_type, A, stats, (TD*)dgrad, ldd, grad_scale_dev,
                       grad_scale_host, loss_scale_dev, arg_train, arg_infer);
    return (int)hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------------------ mv_rows_mul
// One wave per output row, 4 columns per lane per step.  A negative row index (a position mv_pack_plan dropped) yields zeros.
template <typename T>
__global__ __launch_bounds__(256) void rows_mul_kernel(const T* __restrict__ a, int lda, const int32_t* __restrict__ ra,
                                                       const T* __restrict__ b, int ldb, const int32_t* __restrict__ rb, int R, int H,
                                                       T* __restrict__ out, int ldo) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= R) return;
  const int ia = ra[i], ib = rb[i];
  T* o = out + (size_t)i * ldo;
  for (int c = lane * 4; c < H; c += 256) {
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ia >= 0 && ib >= 0) v = ld4<T>(a + (size_t)ia * lda + c) * ld4<T>(b + (size_t)ib * ldb + c);
    st4<T>(o + c, v);
  }
}

extern "C" int mv_rows_mul(int dtype, const void* a, int lda, const int32_t* rows_a, const void* b, int ldb, const int32_t* rows_b, int R,
                           int H, void* out, int ldo, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !b || !rows_a || !rows_b || !out || R <= 0 || H <= 0) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if ((H & 3) || (lda & 3) || (ldb & 3) || (ldo & 3) || lda < H || ldb < H || ldo < H) return MV_E_SHAPE;
  const uintptr_t al = (uintptr_t)(4 * mv_dtype_size(dtype) - 1);
  if ((((uintptr_t)a) & al) || (((uintptr_t)b) & al) || (((uintptr_t)out) & al)) return MV_E_SHAPE;
  const dim3 grid((R + 3) / 4), block(256);
  return mv_with_type(dtype, [&](auto t) -> int {
    typedef MV_T(t) T;
    hipLaunchKernelGGL(rows_mul_kernel<T>, grid, block, 0, stream, (const T*)a, lda, rows_a, (const T*)b, ldb, rows_b, R, H, (T*)out, ldo);
    return (int)hipGetLastError();
  });
}
