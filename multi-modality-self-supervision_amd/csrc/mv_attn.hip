// Fused-mask multi-head attention for the CXRBERT hot path on gfx950.
//
// Replaces HF BertSelfAttention's  softmax(q.k^T/sqrt(dh) + (1-mask)*-10000) . v  and its
// backward (spec: Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/
// model.py:301-320) together with CXRBertEncoder.get_extended_attn_mask
// (models/cxrbert_origin.py:75-85).  The [B,L,L] int64 mask of data/dataset_origin.py:138-176
// is packed once per batch into bits + a per-64x64-tile class (mask_pack kernels) and the
// additive -10000 is applied on the fly; the [B,A,L,L] score tensor never exists in HBM.
//
// MFMA kernels (bf16, dh = 64), all on v_mfma_f32_32x32x16_bf16, flash-style:
//   forward : one wave = 32 queries ON THE LANES (S^T = K.Q^T, O^T = V^T.P^T) so that the
//             running max / sum / rescale are lane-local; P^T goes from the accumulator
//             straight into the next MFMA's B operand (no LDS round trip).
//   dQ      : same orientation (dS^T is lane-local in q, dQ^T = K^T.dS^T).
//   dK,dV   : one wave = 32 keys on the lanes (S = Q.K^T, dV^T = dO^T.P, dK^T = Q^T.dS).
// K/V (or Q/dO) tiles of 64 rows x 64 dh live in LDS in ONE image that serves both the
// row reads (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16), conflict-free for both.
// The VALU kernels are the exact-fp32 path and the on-GPU cross-check.
//
// Files: mv_attn.h        what more than one unit uses (arguments, tile image, LDS-DMA, fragments, tile masks, keep-bits, host helpers)
//        mv_attn_mask.hip  mask packing, tile classes, the dropout keep-bit generator  (mv_mask_pack, mv_mask_build, mv_attn_dropmask)
//        mv_attn_mfma.hip  the three MFMA kernels and their launchers (one unit: they share the ring and the phase profile's counters)
//        mv_attn_simple.hip the VALU kernels and their launchers
//        mv_attn_probs.hip attention probabilities, MFMA and VALU  (mv_attn_probs)
//        mv_attn.hip       this file: mv_attn_fwd and mv_attn_bwd -- validation, the MFMA kernels' arguments, the choice between MFMA and VALU
#include "mv_attn.h"

// what mv_attn_fwd and mv_attn_bwd both put into the MFMA kernels' arguments
static AttnArgs attn_args(const void* qkv, const uint32_t* bits, const uint8_t* tileinfo, int B, int L, int A, int dh, size_t bytes_qkv, float p_drop,
                          const uint32_t* dropbits, const int32_t* cu, const int32_t* qlim) {
  AttnArgs a{};
  attn_fill_common(a, B, L, A, dh, p_drop, dropbits);
  a.cu = cu; a.qlim = qlim; a.order = mv_knob(MV_KNOB_ATTN_ORDER);
  a.qkv = (const bf16_t*)qkv; a.bits = bits; a.info = tileinfo;
  a.T = (L + 63) / 64;
  a.bytes_qkv = (unsigned)bytes_qkv;
  a.drop_on = p_drop > 0.f; a.bytes_dbits = (unsigned)(dropbits_words(B, L, A) * 4);
  return a;
}

extern "C" int mv_attn_fwd(int dtype, const void* qkv, const uint32_t* bits, const uint8_t* tileinfo, void* ctx, void* ctx_bf16,
                           float* lse, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits,
                           const int32_t* cu, int total_rows, const int32_t* qlim, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!qkv || !bits || !tileinfo || !ctx || !lse || B <= 0 || L <= 0 || A <= 0 || dh <= 0) return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  if (ctx_bf16 && dtype != MV_F16) return MV_E_DTYPE;     // the second context output is the bf16 copy of an f16 forward
  const int rcd = dropbits_check(p_drop, dropbits, B, L, A);
  if (rcd) return rcd;
  const int H = A * dh;
  if (mv_is16(dtype) && g_mv_impl == 0) {
    if (dh != 64) return MV_E_SHAPE;
    if (cu && (total_rows <= 0 || total_rows > B * L)) return MV_E_ARG;
    const size_t nrow = cu ? (size_t)total_rows : (size_t)B * L;
    const size_t bq = nrow * 3 * H * 2;
    if (bq >= 0x7fffffffULL || (((uintptr_t)qkv) & 15) || (((uintptr_t)ctx) & 7) || (((uintptr_t)ctx_bf16) & 7)) return MV_E_SHAPE;
    AttnArgs a = attn_args(qkv, bits, tileinfo, B, L, A, dh, bq, p_drop, dropbits, cu, qlim);
    a.out = (bf16_t*)ctx; a.out2 = (bf16_t*)ctx_bf16; a.lse = lse;
    return mv_attn_launch_fwd(a, dtype == MV_F16, stream);      // both 16-bit encodings travel as bf16_t pointers
  }
  if (dh > 128 || cu || qlim) return MV_E_SHAPE;       // packed rows / query limits: MFMA kernels only
  int rc = mv_attn_simple_fwd(dtype, qkv, bits, ctx, lse, B, L, A, dh, p_drop, dropbits, stream);
  // VALU cross-check of the f16 forward (mv_set_impl(1)): ctx_bf16 comes with MV_F16 only (checked above)
  if (rc == MV_OK && ctx_bf16) rc = mv_cast(ctx, MV_F16, ctx_bf16, MV_BF16, (size_t)B * L * H, stream_);
  return rc;
}

extern "C" int mv_attn_bwd(int dtype, const void* qkv, const void* ctx, const void* dctx, const float* lse, const uint32_t* bits,
                           const uint8_t* tileinfo, void* dqkv, float* delta, int B, int L, int A, int dh, float p_drop,
                           const uint32_t* dropbits, const int32_t* cu, int total_rows, const int32_t* qlim, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!qkv || !ctx || !dctx || !lse || !bits || !tileinfo || !dqkv || !delta || B <= 0 || L <= 0 || A <= 0 || dh <= 0)
    return MV_E_ARG;
  if (!mv_dtype_ok(dtype)) return MV_E_DTYPE;
  const int rcd = dropbits_check(p_drop, dropbits, B, L, A);
  if (rcd) return rcd;
  const int H = A * dh;
  if (mv_is16(dtype) && g_mv_impl == 0) {
    if (dh != 64) return MV_E_SHAPE;
    if (cu && (total_rows <= 0 || total_rows > B * L)) return MV_E_ARG;
    const size_t nrow = cu ? (size_t)total_rows : (size_t)B * L;
    const size_t bq = nrow * 3 * H * 2, bc = nrow * H * 2;
    if (bq >= 0x7fffffffULL || (((uintptr_t)qkv) & 15) || (((uintptr_t)dctx) & 15) || (((uintptr_t)dqkv) & 7)) return MV_E_SHAPE;
    AttnArgs a = attn_args(qkv, bits, tileinfo, B, L, A, dh, bq, p_drop, dropbits, cu, qlim);
    a.ctx = (const bf16_t*)ctx; a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv;
    a.lse_in = lse; a.delta = delta; a.delta_out = delta;
    a.bytes_ctx = (unsigned)bc;
    a.bytes_stat = (unsigned)((size_t)B * A * L * 4); a.bytes_bits = (unsigned)((size_t)B * L * a.W * 4);
    return mv_attn_launch_bwd(a, dtype == MV_F16, stream);
  }
  if (dh > 128 || cu || qlim) return MV_E_SHAPE;
  return mv_attn_simple_bwd(dtype, qkv, ctx, dctx, lse, bits, dqkv, delta, B, L, A, dh, p_drop, dropbits, stream);
}
