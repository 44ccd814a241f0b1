"""Tensor-level wrappers over the C ABI (include/medvill.h).  torch is used for device memory
and streams only; every wrapper enqueues on torch's current stream and returns immediately."""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_D, EPI_BIAS_RELU, EPI_BIAS_RES, EPI_BIAS_RES_RELU, EPI_BIAS_TANH, EPI_DGELU,  # noqa: F401
                   EPI_MUL, EPI_NONE, EPI_RES, MV_BF16, MV_F16,
                   MV_F32)


def _lib():
    return L.load()


def gemm(a, b, c, *, ta=False, tb=False, M, N, K, lda=None, ldb=None, ldc=None, bias=None, epi=EPI_NONE, r=None, ldr=None,
         c2=None, ldc2=None, c3=None, ldc3=None, splitk=1, ws=None, accumulate=False, p_drop=0.0, drop_key=0, alpha=None, colsum_part=None):
    """c[M,N] = epi(op(a)[M,K] . op(b)[K,N]); c3 (optional): the same result in a second 16-bit encoding; alpha (optional,
    f32 device scalar): factor on the product (weight gradients of the f16-gradient path); see mv_gemm in include/medvill.h."""
    L.require_cuda(a, b, c, bias, r, c2, c3, ws, alpha, colsum_part)
    if colsum_part is not None and (colsum_part.dtype != torch.float32 or colsum_part.numel() < 2 * ((M + 255) // 256) * N):
        raise ValueError("colsum_part: f32 [2*ceil(M/256), N]")
    lda = lda if lda is not None else (M if ta else K)
    ldb = ldb if ldb is not None else (N if tb else K)
    ldc = ldc if ldc is not None else N
    ldr = ldr if ldr is not None else N
    ldc2 = ldc2 if ldc2 is not None else N
    ldc3 = ldc3 if ldc3 is not None else N
    if a.dtype != b.dtype:
        raise TypeError("gemm operands must share a dtype")
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("bias must be f32")
    rc = _lib().mv_gemm(L.dt_of(a), int(ta), int(tb), M, N, K, L.ptr(a), lda, L.ptr(b), ldb, L.ptr(c), ldc, L.dt_of(c),
                        L.ptr(bias), epi, L.ptr(r), ldr, L.dt_of(r) if r is not None else 0, L.ptr(c2), ldc2,
                        L.ptr(c3), ldc3, L.dt_of(c3) if c3 is not None else 0, splitk, L.ptr(ws), (ws.numel() * 4) if ws is not None else 0, int(accumulate), float(p_drop), int(drop_key),
                        L.ptr(alpha), L.ptr(colsum_part), L.stream_ptr())
    L.check(rc, f"mv_gemm(M={M},N={N},K={K},ta={ta},tb={tb},epi={epi})")
    return c


def mask_pack(mask, bits, tileinfo):
    L.require_cuda(mask, bits, tileinfo)
    if mask.dtype != torch.int64:
        raise TypeError("attn_mask must be int64 (as built by the reference Dataset)")
    if mask.dim() not in (2, 3):
        raise NotImplementedError          # cxrbert_origin.py:80-81
    B, Lq = mask.shape[0], mask.shape[-1]
    rc = _lib().mv_mask_pack(L.ptr(mask.contiguous()), mask.dim(), B, Lq, L.ptr(bits), L.ptr(tileinfo), L.stream_ptr())
    L.check(rc, "mv_mask_pack")


def mask_build(desc, B, Lq, bits, tileinfo):
    """bits / tile classes from int32 [B,3] descriptors {family, n2, vl} (see mv_mask_build)."""
    L.require_cuda(desc, bits, tileinfo)
    if desc.dtype != torch.int32 or tuple(desc.shape) != (B, 3):
        raise TypeError("desc must be int32 [B,3]")
    rc = _lib().mv_mask_build(L.ptr(desc.contiguous()), B, Lq, L.ptr(bits), L.ptr(tileinfo), L.stream_ptr())
    L.check(rc, "mv_mask_build")


def mask_verify_host(mask, desc, threads=4):
    """HOST tensors: int64 [B,L,L] / [B,L] reference mask against int32 [B,3] descriptors (see mv_mask_verify_host).
    -> -1 when every entry agrees, else the linear index of the first mismatch.  Pure host work; releases the GIL."""
    import ctypes
    if mask.is_cuda or desc.is_cuda or mask.dtype != torch.int64 or desc.dtype != torch.int32:
        raise TypeError("mask_verify_host: host int64 mask and host int32 [B,3] descriptors")
    if mask.dim() not in (2, 3):
        raise NotImplementedError          # cxrbert_origin.py:80-81
    B, Lq = mask.shape[0], mask.shape[-1]
    if tuple(desc.shape) != (B, 3):
        raise TypeError("desc must be int32 [B,3]")
    mask, desc = mask.contiguous(), desc.contiguous()
    out = ctypes.c_longlong(0)
    rc = _lib().mv_mask_verify_host(mask.data_ptr(), mask.dim(), desc.data_ptr(), B, Lq, int(threads), ctypes.byref(out))
    L.check(rc, "mv_mask_verify_host")
    return int(out.value)


def mlm_draws(key, B, S, vocab, device):
    """(u f32 [B,S], rnd int32 [B,S]): the counter-based stand-ins for random_word's two random sources."""
    u = torch.empty((B, S), dtype=torch.float32, device=device)
    rnd = torch.empty((B, S), dtype=torch.int32, device=device)
    L.require_cuda(u)
    rc = _lib().mv_mlm_draws(int(key) & 0xFFFFFFFFFFFFFFFF, B, S, vocab, L.ptr(u), L.ptr(rnd), L.stream_ptr())
    L.check(rc, "mv_mlm_draws")
    return u, rnd


def mlm_corrupt(ids, lengths, u, rnd, N, family=None, want_index=True):
    """On-device sample assembly (see mv_mlm_corrupt).  Returns a dict of device tensors; `n_labels` stays on the
    device (one int32) so the caller decides when to synchronise."""
    L.require_cuda(ids, lengths, u, rnd, family)
    B, S = ids.shape
    T, Lq = S + 1, S + N + 3
    if ids.dtype != torch.int64 or lengths.dtype != torch.int32 or u.dtype != torch.float32 or rnd.dtype != torch.int32:
        raise TypeError("mlm_corrupt: ids int64, lengths int32, u f32, rnd int32")
    if tuple(lengths.shape) != (B,) or tuple(u.shape) != (B, S) or tuple(rnd.shape) != (B, S):
        raise ValueError("mlm_corrupt: shape mismatch")
    if family is not None and (family.dtype != torch.int32 or tuple(family.shape) != (B,)):
        raise TypeError("mlm_corrupt: family must be int32 [B]")
    dev = ids.device
    out = dict(input_txt=torch.empty((B, T), dtype=torch.int64, device=dev),
               segment=torch.empty((B, T), dtype=torch.int64, device=dev),
               txt_labels=torch.empty((B, Lq), dtype=torch.int64, device=dev),
               n_ids=torch.empty((B,), dtype=torch.int32, device=dev),
               desc=torch.empty((B, 3), dtype=torch.int32, device=dev),
               counts=torch.empty((B,), dtype=torch.int32, device=dev))
    if want_index:
        out["label_rows"] = torch.empty((B * S,), dtype=torch.int32, device=dev)
        out["label_ids"] = torch.empty((B * S,), dtype=torch.int32, device=dev)
        out["n_labels"] = torch.empty((1,), dtype=torch.int32, device=dev)
    rc = _lib().mv_mlm_corrupt(L.ptr(ids.contiguous()), L.ptr(lengths.contiguous()), L.ptr(u.contiguous()), L.ptr(rnd.contiguous()),
                               L.ptr(family), B, N, S, L.ptr(out["input_txt"]), L.ptr(out["segment"]), L.ptr(out["txt_labels"]),
                               L.ptr(out["n_ids"]), L.ptr(out["desc"]), L.ptr(out["counts"]), L.ptr(out.get("label_rows")),
                               L.ptr(out.get("label_ids")), L.ptr(out.get("n_labels")), L.stream_ptr())
    L.check(rc, "mv_mlm_corrupt")
    return out


def pack_plan(desc, B, Lq):
    """(cu int32 [B+1], rowmap int32 [B*L], inv int32 [B*L]) from mask descriptors (see mv_pack_plan); device tensors."""
    L.require_cuda(desc)
    if desc.dtype != torch.int32 or tuple(desc.shape) != (B, 3):
        raise TypeError("desc must be int32 [B,3]")
    dev = desc.device
    cu = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    rowmap = torch.empty((B * Lq,), dtype=torch.int32, device=dev)
    inv = torch.empty((B * Lq,), dtype=torch.int32, device=dev)
    rc = _lib().mv_pack_plan(L.ptr(desc.contiguous()), B, Lq, L.ptr(cu), L.ptr(rowmap), L.ptr(inv), L.stream_ptr())
    L.check(rc, "mv_pack_plan")
    return cu, rowmap, inv


def tail_perm(cu, B, Lq, sel, total_rows):
    """(perm, newpos, qlim, sel_new) of mv_tail_perm: the last layer's row order with the consumed rows `sel` (packed row indices) first.
    sel_new is -1 where sel names no row (the -1 of a dropped position, or an index >= total_rows): the kernel writes every entry."""
    L.require_cuda(cu, sel)
    if cu.dtype != torch.int32 or sel.dtype != torch.int32:
        raise TypeError("tail_perm: int32 tensors")
    dev = cu.device
    perm = torch.empty((total_rows,), dtype=torch.int32, device=dev)
    newpos = torch.empty((total_rows,), dtype=torch.int32, device=dev)
    qlim = torch.empty((B,), dtype=torch.int32, device=dev)
    sel_new = torch.empty((sel.numel(),), dtype=torch.int32, device=dev)
    rc = _lib().mv_tail_perm(L.ptr(cu), B, Lq, L.ptr(sel.contiguous()), int(sel.numel()), L.ptr(perm), L.ptr(newpos), L.ptr(qlim), L.ptr(sel_new),
                             L.stream_ptr())
    L.check(rc, "mv_tail_perm")
    return perm, newpos, qlim, sel_new


def dropbits_numel(B, Lq, A):
    """uint32 elements of one layer's attention-dropout keep-bits (mv_attn_dropmask)."""
    return B * A * ((Lq + 31) // 32) * ((Lq + 63) // 64) * 64


def attn_dropmask(p_drop, drop_key, B, Lq, A, out, cu=None):
    """Keep-bits of the attention-probability dropout mask of (p_drop, drop_key), in the layout the MFMA kernels select with."""
    L.require_cuda(out, cu)
    if out.dtype != torch.int32 or out.numel() < dropbits_numel(B, Lq, A):
        raise TypeError("attn_dropmask: out must be int32 with dropbits_numel(B, L, A) elements")
    rc = _lib().mv_attn_dropmask(float(p_drop), int(drop_key), B, Lq, A, L.ptr(cu), L.ptr(out), L.stream_ptr())
    L.check(rc, "mv_attn_dropmask")
    return out


def attn_keep_mask(dropbits, B, Lq, A):
    """The keep-bits of mv_attn_dropmask decoded to a bool tensor [B, A, L, L] (keep[b, h, q, k]) -- inspection / tests.  Blocks the
    generator skipped (beyond a sample's packed length) decode to whatever the buffer held."""
    NQB, NKT = (Lq + 31) // 32, (Lq + 63) // 64
    w = dropbits[:dropbits_numel(B, Lq, A)].view(B, A, NQB, NKT, 2, 16, 2).to(torch.int64) & 0xFFFFFFFF     # [b, h, qb, kt, kk, r, half]
    i = torch.arange(32, device=dropbits.device, dtype=torch.int64)
    bit = ((w.unsqueeze(-1) >> i) & 1).bool()                      # [..., r, half, query-in-block]
    r = torch.arange(16, device=dropbits.device)
    key_of = ((r & 3) + 8 * (r >> 2)).view(16, 1) + 4 * torch.arange(2, device=dropbits.device).view(1, 2)      # [r, half] -> key in the 32-half
    out = torch.zeros((B, A, NQB, NKT, 2, 32, 32), dtype=torch.bool, device=dropbits.device)             # [.., kk, key32, q32]
    out[:, :, :, :, :, key_of.reshape(-1), :] = bit.reshape(B, A, NQB, NKT, 2, 32, 32)
    # -> [b, h, qb, q32, kt, kk, key32]
    out = out.permute(0, 1, 2, 6, 3, 4, 5).reshape(B, A, NQB * 32, NKT * 64)
    return out[:, :, :Lq, :Lq]


def attn_fwd(qkv, bits, tileinfo, ctx, lse, B, Lq, A, dh, p_drop=0.0, cu=None, total_rows=0, ctx_bf16=None, dropbits=None, qlim=None):
    """p_drop > 0 needs `dropbits` (attn_dropmask).  qlim (int32 [B], optional): only the first qlim[b] rows of a sample are queries."""
    if ctx.dtype != qkv.dtype or (ctx_bf16 is not None and ctx_bf16.dtype != torch.bfloat16):
        raise TypeError("attn_fwd: ctx shares qkv's encoding; the second output is bf16")
    L.require_cuda(dropbits)
    rc = _lib().mv_attn_fwd(L.dt_of(qkv), L.ptr(qkv), L.ptr(bits), L.ptr(tileinfo), L.ptr(ctx), L.ptr(ctx_bf16), L.ptr(lse), B, Lq, A, dh,
                            float(p_drop), L.ptr(dropbits), L.ptr(cu), int(total_rows), L.ptr(qlim), L.stream_ptr())
    L.check(rc, "mv_attn_fwd")


def attn_probs(qkv, bits, tileinfo, lse, out, B, Lq, A, dh, p_drop=0.0, dropbits=None, head_mean=False):
    """The layer's attention probabilities (see mv_attn_probs) into `out`: [B, A, L, L], or [B, L, L] with head_mean; f32 or qkv's
    encoding.  Dense rows only; p_drop > 0 applies the layer's keep-bits `dropbits`."""
    L.require_cuda(qkv, bits, tileinfo, lse, out, dropbits)
    n = B * (1 if head_mean else A) * Lq * Lq
    if out.dtype not in (torch.float32, qkv.dtype) or out.numel() != n or not out.is_contiguous():
        raise TypeError("attn_probs: out must be a contiguous f32 (or qkv-encoded) tensor of B*A*L*L elements (B*L*L with head_mean)")
    if lse.dtype != torch.float32 or lse.numel() < B * A * Lq:
        raise TypeError("attn_probs: lse must be f32 [B, A, L]")
    rc = _lib().mv_attn_probs(L.dt_of(qkv), L.ptr(qkv), L.ptr(bits), L.ptr(tileinfo), L.ptr(lse), L.ptr(out), L.dt_of(out), B, Lq, A, dh,
                              float(p_drop), L.ptr(dropbits), int(bool(head_mean)), L.stream_ptr())
    L.check(rc, "mv_attn_probs")
    return out


def attn_bwd(qkv, ctx, dctx, lse, bits, tileinfo, dqkv, delta, B, Lq, A, dh, p_drop=0.0, cu=None, total_rows=0, dropbits=None, qlim=None):
    L.require_cuda(dropbits, qlim)
    rc = _lib().mv_attn_bwd(L.dt_of(qkv), L.ptr(qkv), L.ptr(ctx), L.ptr(dctx), L.ptr(lse), L.ptr(bits), L.ptr(tileinfo),
                            L.ptr(dqkv), L.ptr(delta), B, Lq, A, dh, float(p_drop), L.ptr(dropbits), L.ptr(cu), int(total_rows),
                            L.ptr(qlim), L.stream_ptr())
    L.check(rc, "mv_attn_bwd")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, M, H, eps, y_bf16=None):
    if y_bf16 is not None and y_bf16.dtype != torch.bfloat16:
        raise TypeError("layernorm_fwd: the second output is bf16")
    rc = _lib().mv_layernorm_fwd(L.dt_of(y), L.ptr(x), L.dt_of(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(y_bf16), L.ptr(mean),
                                 L.ptr(rstd), M, H, float(eps), L.stream_ptr())
    L.check(rc, "mv_layernorm_fwd")


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, colsum, M, H, dx_drop=None, p_drop=0.0, drop_key=0, unscale=None):
    rc = _lib().mv_layernorm_bwd(L.dt_of(dy), L.ptr(dy), L.ptr(x), L.dt_of(x), L.ptr(mean), L.ptr(rstd), L.ptr(gamma),
                                 L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), L.ptr(colsum), M, H, L.ptr(dx_drop), float(p_drop),
                                 int(drop_key), L.ptr(unscale), L.stream_ptr())
    L.check(rc, "mv_layernorm_bwd")


def embed_fwd(dt, cls_tok, txt, segment, img_pos, sep_tok, imgproj, E, P, Ty, gamma, beta, x0, pre, mean, rstd, B, N, T, H, V,
              maxpos, eps, p_drop=0.0, drop_key=0, rowmap=None, n_rows=0, x0_bf16=None, p_drop_img=None):
    """img_pos None: the image rows get no position embedding (args.img_postion false); p_drop_img: dropout probability of the image
    rows (args.dropout_prob, cxrbert_origin.py:19; default = p_drop)."""
    if any(L.dt_of(t) != dt for t in (E, P, Ty, x0)) or (imgproj is not None and L.dt_of(imgproj) != dt):
        raise TypeError("embed_fwd: tables, imgproj and x0 must be in the encoding `dt`")
    rc = _lib().mv_embed_fwd(dt, L.ptr(cls_tok), L.ptr(txt), L.ptr(segment), L.ptr(img_pos), L.ptr(sep_tok), L.ptr(imgproj),
                             L.ptr(E), L.ptr(P), L.ptr(Ty), L.ptr(gamma), L.ptr(beta), L.ptr(x0), L.ptr(x0_bf16), L.ptr(pre), L.ptr(mean),
                             L.ptr(rstd), B, N, T, H, V, maxpos, float(eps), float(p_drop),
                             float(p_drop if p_drop_img is None else p_drop_img), int(drop_key), L.ptr(rowmap), int(n_rows),
                             L.stream_ptr())
    L.check(rc, "mv_embed_fwd")


def embed_bwd(dt, dx0, pre, mean, rstd, gamma, cls_tok, txt, segment, img_pos, sep_tok, dE, dP, dTy, dgamma, dbeta, dimgproj, B,
              N, T, H, V, maxpos, pad_token_id=0, p_drop=0.0, drop_key=0, rowmap=None, n_rows=0, unscale=None, p_drop_img=None):
    rc = _lib().mv_embed_bwd(dt, L.ptr(dx0), L.ptr(pre), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(cls_tok), L.ptr(txt),
                             L.ptr(segment), L.ptr(img_pos), L.ptr(sep_tok), L.ptr(dE), L.ptr(dP), L.ptr(dTy), L.ptr(dgamma),
                             L.ptr(dbeta), L.ptr(dimgproj), B, N, T, H, V, maxpos, int(pad_token_id), float(p_drop),
                             float(p_drop if p_drop_img is None else p_drop_img), int(drop_key),
                             L.ptr(rowmap), int(n_rows), L.ptr(unscale), L.stream_ptr())
    L.check(rc, "mv_embed_bwd")


def ce_fwd_bwd(logits, ld, labels, R, V, out, dlogits=None, ldd=0, grad_scale_dev=None, grad_scale=1.0, loss_scale_dev=None):
    if labels.dtype != torch.int32:
        raise TypeError("labels must be int32")
    rc = _lib().mv_ce_fwd_bwd(L.ptr(logits), L.dt_of(logits), ld, L.ptr(labels), R, V, L.ptr(out), L.ptr(dlogits),
                              L.dt_of(dlogits) if dlogits is not None else 0, ldd, L.ptr(grad_scale_dev), float(grad_scale),
                              L.ptr(loss_scale_dev), L.stream_ptr())
    L.check(rc, "mv_ce_fwd_bwd")


def gather_rows(src, lds, rows, R, H, dst, ldd):
    rc = _lib().mv_gather_rows(L.dt_of(src), L.ptr(src), lds, L.ptr(rows), R, H, L.ptr(dst), ldd, L.stream_ptr())
    L.check(rc, "mv_gather_rows")


def scatter_rows(src, lds, rows, R, H, dst, ldd, accumulate=False):
    rc = _lib().mv_scatter_rows(L.dt_of(src), L.ptr(src), lds, L.ptr(rows), R, H, L.ptr(dst), ldd, int(accumulate),
                                L.stream_ptr())
    L.check(rc, "mv_scatter_rows")


def colsum(x, ldx, M, N, out, accumulate=True, unscale=None):
    rc = _lib().mv_colsum(L.dt_of(x), L.ptr(x), ldx, M, N, L.ptr(out), int(accumulate), L.ptr(unscale), L.stream_ptr())
    L.check(rc, "mv_colsum")


def colsum_partials(part, P, ld, N, out, unscale=None):
    """out[n] += [unscale] * sum_p part[p, n] (the partial column sums of gemm(colsum_part=))."""
    L.require_cuda(part, out, unscale)
    rc = _lib().mv_colsum_partials(L.ptr(part), P, ld, N, L.ptr(out), L.ptr(unscale), L.stream_ptr())
    L.check(rc, "mv_colsum_partials")


def add(a, b, c, n):
    rc = _lib().mv_add(L.dt_of(a), L.ptr(a), L.ptr(b), L.ptr(c), n, L.stream_ptr())
    L.check(rc, "mv_add")


def dact(mode, dy, z, out, n):
    rc = _lib().mv_dact(L.dt_of(dy), mode, L.ptr(dy), L.ptr(z), L.ptr(out), n, L.stream_ptr())
    L.check(rc, "mv_dact")


def cast(src, dst, n):
    rc = _lib().mv_cast(L.ptr(src), L.dt_of(src), L.ptr(dst), L.dt_of(dst), n, L.stream_ptr())
    L.check(rc, "mv_cast")


def transpose(src, dst, rows, cols, lds=None, ldd=None):
    """dst[c, r] = src[r, c] (same dtype)."""
    L.require_cuda(src, dst)
    if src.dtype != dst.dtype:
        raise TypeError("transpose: dtypes differ")
    rc = _lib().mv_transpose(L.dt_of(src), L.ptr(src), lds if lds is not None else cols, L.ptr(dst), ldd if ldd is not None else rows,
                             rows, cols, L.stream_ptr())
    L.check(rc, "mv_transpose")
    return dst


def nchw_to_nhwc(src, dst, B, C, H, W, Cp):
    L.require_cuda(src, dst)
    if src.dtype != torch.float32:
        raise TypeError("nchw_to_nhwc: source pixels must be float32")
    rc = _lib().mv_nchw_to_nhwc(L.ptr(src), L.ptr(dst), L.dt_of(dst), B, C, H, W, Cp, L.stream_ptr())
    L.check(rc, "mv_nchw_to_nhwc")


def im2col(src, dst, B, H, W, C, kh, kw, stride, pad, ldk):
    L.require_cuda(src, dst)
    rc = _lib().mv_im2col(L.dt_of(src), L.ptr(src), B, H, W, C, kh, kw, stride, pad, L.ptr(dst), ldk, L.stream_ptr())
    L.check(rc, "mv_im2col")


def conv2d(x, w, y, B, H, W, C, O, kh, kw, stride, pad, bias=None, epi=EPI_NONE, r=None):
    """implicit-GEMM convolution over NHWC x [B*H*W, C] with w [O, kh*kw*C] -> y [B*Ho*Wo, O] (see mv_conv2d)."""
    L.require_cuda(x, w, y, bias, r)
    rc = _lib().mv_conv2d(L.dt_of(x), L.ptr(x), L.ptr(w), L.ptr(y), L.dt_of(y), B, H, W, C, O, kh, kw, stride, pad, L.ptr(bias), epi,
                          L.ptr(r), L.dt_of(r) if r is not None else 0, L.stream_ptr())
    L.check(rc, "mv_conv2d")


def col_stats(x, ldx, rows, C, stats):
    L.require_cuda(x, stats)
    rc = _lib().mv_col_stats(L.dt_of(x), L.ptr(x), ldx, rows, C, L.ptr(stats), L.stream_ptr())
    L.check(rc, "mv_col_stats")


def bn_finalize(stats, C, rows, eps, momentum, mean, rstd, running_mean=None, running_var=None):
    L.require_cuda(stats, mean, rstd, running_mean, running_var)
    rc = _lib().mv_bn_finalize(L.ptr(stats), C, int(rows), float(eps), float(momentum), L.ptr(mean), L.ptr(rstd),
                               L.ptr(running_mean), L.ptr(running_var), L.stream_ptr())
    L.check(rc, "mv_bn_finalize")


def bn_act(x, mean, rstd, gamma, beta, y, rows, C, residual=None, relu=True):
    L.require_cuda(x, mean, rstd, gamma, beta, y, residual)
    rc = _lib().mv_bn_act(L.dt_of(y), L.ptr(x), L.dt_of(x), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(beta), L.ptr(residual), L.ptr(y),
                          int(rows), C, int(relu), L.stream_ptr())
    L.check(rc, "mv_bn_act")


def maxpool3x3s2(x, y, B, H, W, C):
    L.require_cuda(x, y)
    rc = _lib().mv_maxpool3x3s2(L.dt_of(x), L.ptr(x), L.ptr(y), B, H, W, C, L.stream_ptr())
    L.check(rc, "mv_maxpool3x3s2")


def cast2d(src, lds, dst, ldd, rows, cols):
    rc = _lib().mv_cast2d(L.ptr(src), L.dt_of(src), lds, L.ptr(dst), L.dt_of(dst), ldd, rows, cols, L.stream_ptr())
    L.check(rc, "mv_cast2d")


def adamw_step(p, g, m, v, shadow, n, lr, b1, b2, eps, wd, step, correct_bias=True, grad_scale=1.0, shadow_f16=None, scaler_state=None):
    rc = _lib().mv_adamw_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(shadow), L.ptr(shadow_f16), n, float(lr), float(b1), float(b2),
                              float(eps), float(wd), int(step), int(correct_bias), float(grad_scale), L.ptr(scaler_state), L.stream_ptr())
    L.check(rc, "mv_adamw_step")


def count_nonfinite(x, counter):
    """counter[0] += number of inf / nan elements of the f32 tensor x (device)."""
    L.require_cuda(x, counter)
    if x.dtype != torch.float32 or counter.dtype != torch.float32:
        raise TypeError("count_nonfinite: f32 tensors")
    rc = _lib().mv_count_nonfinite(L.ptr(x), x.numel(), L.ptr(counter), L.stream_ptr())
    L.check(rc, "mv_count_nonfinite")


def scaler_update(state, growth_interval=2000, growth=2.0, backoff=0.5, max_scale=2.0 ** 24, min_scale=1.0):
    """Dynamic loss scale: consume the non-finite count in state[6], set the skip flag / step count, adapt the scale."""
    L.require_cuda(state)
    rc = _lib().mv_scaler_update(L.ptr(state), int(growth_interval), float(growth), float(backoff), float(max_scale), float(min_scale),
                                 L.stream_ptr())
    L.check(rc, "mv_scaler_update")


def dropout_mask(p_drop, drop_key, n, device):
    """(keep uint8 [n], scale) of the kernels' counter-based dropout for linear indices 0..n-1."""
    import ctypes
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    sc = ctypes.c_float(1.0)
    rc = _lib().mv_dropout_mask(float(p_drop), int(drop_key), n, L.ptr(keep), ctypes.byref(sc), L.stream_ptr())
    L.check(rc, "mv_dropout_mask")
    return keep, float(sc.value)


# ---- kernel-forcing knobs: tests and timing experiments only (include/medvill_debug.h).  The product library has none of this state;
# a knob off its default routes the process's calls through libmedvill_hip_dbg.so (medvill_amd._lib.set_knob). ----
def set_impl(impl: int):
    L.set_knob("impl", 1 if impl else 0)


def get_impl() -> int:
    return L.get_knob("impl")


def set_attn_planes(planes: int):
    """Bits per uniform of the attention-dropout mask generator (16, 12 or 8)."""
    L.set_knob("attn_planes", planes if planes in (8, 12) else 16)


def attn_drop_prob(p_drop: float) -> float:
    """The drop probability attn_dropmask realises for p_drop at the current plane count."""
    n = L.get_knob("attn_planes")
    return round(p_drop * (1 << n)) / float(1 << n)


def set_rowops_variant(v: int = 0):
    """Experiment hook of mv_layernorm_bwd (see include/medvill_debug.h)."""
    L.set_knob("rowops_variant", v)


def set_gemm_rounds(on: int = 1):
    """1 (default): mv_gemm picks the ring tile height that minimises whole rounds of CUs (csrc/mv_gemm_plan.h: mv_gemm_plan); 0: off."""
    L.set_knob("gemm_rounds", 1 if on else 0)


def set_attn_fwd(variant: int = 0):
    """Reserved: selects the two-sub-tile forward kernel when profiles/r05_two_subtile_attention_experiment.patch is applied."""
    L.set_knob("attn_fwd", variant)


def set_attn_order(order: int = 0):
    """Attention block order (see att_block in csrc/mv_attn.h): 0 row block slowest, 1 a pair's row blocks adjacent on one XCD."""
    L.set_knob("attn_order", order)


class RcclComm:
    """The C ABI's own RCCL communicator (mv_comm_*: include/medvill.h), for hosts that do not go through torch.distributed.
    `medvill_amd.dist.GradAllReducer` (the product's exchange) uses torch's nccl backend instead -- the same library, one communicator
    per process.  unique_id(): rank 0 makes the 128-byte id and hands it to the other ranks by any transport."""

    def __init__(self, rank: int, world: int, unique_id: bytes):
        import ctypes
        if len(unique_id) != 128:
            raise ValueError("unique_id: 128 bytes (RcclComm.unique_id() on rank 0)")
        self._h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        L.check(_lib().mv_comm_init(ctypes.byref(self._h), int(rank), int(world), buf), "mv_comm_init")
        self.rank, self.world = rank, world

    @staticmethod
    def unique_id() -> bytes:
        import ctypes
        buf = ctypes.create_string_buffer(128)
        L.check(_lib().mv_comm_unique_id(buf), "mv_comm_unique_id")
        return buf.raw

    def allreduce_async(self, t, stream=None):
        """In-place sum all-reduce of a contiguous f32 / f16 / bf16 device tensor, enqueued on `stream` (default: the current one)."""
        L.require_cuda(t)
        if not t.is_contiguous():
            raise ValueError("allreduce_async: contiguous tensor")
        st = (stream or torch.cuda.current_stream()).cuda_stream
        L.check(_lib().mv_comm_allreduce_async(self._h, L.ptr(t), t.numel(), L.dt_of(t), st), "mv_comm_allreduce_async")

    def wait(self, stream=None):
        """`stream` (default: the current one) waits on the device for every collective issued so far."""
        st = (stream or torch.cuda.current_stream()).cuda_stream
        L.check(_lib().mv_comm_wait(self._h, st), "mv_comm_wait")

    def destroy(self):
        if self._h:
            L.check(_lib().mv_comm_destroy(self._h), "mv_comm_destroy")
            self._h = None


def set_persistent_cus(n: int = 0):
    """The persistent (weight-gradient) GEMM kernels launch at most n blocks; 0 = one per CU."""
    L.set_knob("persistent_cus", max(int(n), 0))


def stream_with_cus(n_cus: int, device, first: int = 0, total: int = 256, n_xcd: int = 8):
    """torch stream whose kernels only run on `n_cus` compute units (a multiple of n_xcd: n_cus / n_xcd CUs of every XCD), starting at
    CU `first` (also a multiple of n_xcd).  Bit i of the mask is CU i // n_xcd of XCD i % n_xcd (see mv_stream_create_cumask)."""
    import ctypes
    if n_cus % n_xcd or first % n_xcd or n_cus <= 0 or first + n_cus > total:
        raise ValueError("n_cus and first must be multiples of the XCD count and fit the device")
    words = (ctypes.c_uint32 * ((total + 31) // 32))()
    for i in range(first, first + n_cus):
        words[i // 32] |= 1 << (i % 32)
    out = ctypes.c_void_p()
    with torch.cuda.device(device):
        L.check(_lib().mv_stream_create_cumask(words, len(words), ctypes.byref(out)), "mv_stream_create_cumask")
    return torch.cuda.ExternalStream(out.value, device=device)


def gemm_workspace_bytes(dtype, ta, tb, M, N, K) -> int:
    """Bytes of split-K workspace mv_gemm(splitk=0) would like for this product (0: it never splits); see include/medvill.h."""
    dt = dtype if isinstance(dtype, int) else {torch.float32: MV_F32, torch.bfloat16: MV_BF16, torch.float16: MV_F16}[dtype]
    return int(_lib().mv_gemm_workspace_bytes(dt, int(ta), int(tb), int(M), int(N), int(K)))


def workspace_bytes(hidden, intermediate, vocab, img_hidden, max_rows, max_label_rows, max_regions) -> int:
    """The largest split-K workspace any GEMM of a pretraining step asks for at this geometry (mv_workspace_bytes)."""
    return int(_lib().mv_workspace_bytes(int(hidden), int(intermediate), int(vocab), int(img_hidden), int(max_rows), int(max_label_rows), int(max_regions)))


class GroupProblem(ctypes.Structure):
    """include/medvill.h: mv_group_problem -- C[No, Ko] (+)= alpha * A[rows, No]^T . B[rows, Ko]."""
    _fields_ = [("A", L.vp), ("B", L.vp), ("C", L.vp), ("lda", L.i32), ("ldb", L.i32), ("ldc", L.i32), ("No", L.i32), ("Ko", L.i32),
                ("rows", L.i32)]


class GroupedTN:
    """The problem table of mv_gemm_grouped_tn: a host copy (what the library validates and plans the grid from) and a device copy (all
    the kernels read; the library cannot check it, so it is only ever written from the host copy, right after that was filled).  set()
    rebuilds both only when a problem changed: a loop over batches of one shape copies nothing per step, one whose packed row count
    changes from batch to batch refills the table (a few KiB through one pinned staging buffer) on every step."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.key = None
        self.count = 0
        self.dtype = 0
        self.host = None          # ctypes buffer
        self.dev = None           # uint8 tensor
        self.staged = None        # pinned uint8 tensor the upload reads, and the event after its last upload
        self.staged_ev = None
        self.uploads = 0          # times the table was rebuilt and copied to the device
        self.launches = 0

    def set(self, dtype, problems, n_blocks=0):
        """problems: (a, b, c, No, Ko, rows, lda, ldb, ldc) with tensors a [rows, lda], b [rows, ldb] (16-bit), c f32 [No, ldc].  Returns True
        when the table was rebuilt (and enqueues its upload on the current stream)."""
        dt = dtype if isinstance(dtype, int) else L.dt_of(torch.empty(0, dtype=dtype))
        key = (dt, int(n_blocks), L.get_knob("persistent_cus"),
               tuple((a.data_ptr(), b.data_ptr(), c.data_ptr(), No, Ko, rows, lda, ldb, ldc) for a, b, c, No, Ko, rows, lda, ldb, ldc in problems))
        if key == self.key:
            return False
        for a, b, c, *_ in problems:
            L.require_cuda(a, b, c)
            if L.dt_of(a) != dt or L.dt_of(b) != dt or c.dtype != torch.float32:
                raise TypeError("grouped dW: 16-bit operands of one encoding, f32 outputs")
        n = len(problems)
        arr = (GroupProblem * max(n, 1))(*[GroupProblem(k[0], k[1], k[2], k[6], k[7], k[8], k[3], k[4], k[5]) for k in key[3]])
        nbytes = int(_lib().mv_gemm_grouped_table_bytes(n))
        host = self.host if self.host is not None and len(self.host) >= nbytes else ctypes.create_string_buffer(max(nbytes, 1))
        self.key = None           # a failed fill leaves no table behind
        L.check(_lib().mv_gemm_grouped_fill(dt, n, arr, int(n_blocks), host, nbytes), f"mv_gemm_grouped_fill(count={n})")
        if self.staged is None or self.staged.numel() < nbytes:
            self.staged = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        elif self.staged_ev is not None:
            self.staged_ev.synchronize()      # the previous upload has read the staging buffer
        ctypes.memmove(self.staged.data_ptr(), host, nbytes)
        self.dev[:nbytes].copy_(self.staged[:nbytes], non_blocking=True)
        self.staged_ev = torch.cuda.Event()
        self.staged_ev.record()
        self.host, self.key, self.count, self.dtype = host, key, n, dt
        self.uploads += 1
        return True

    def workspace_bytes(self) -> int:
        return int(_lib().mv_gemm_grouped_workspace_bytes(self.host))

    def units(self):
        """Every launch unit as (problem, m0, n0, kbeg, kend, slice, tile) -- the kernel's own map (mv_gemm_grouped_decode)."""
        hdr = (ctypes.c_int * 16).from_buffer(self.host)
        out = (ctypes.c_int * 7)()
        res = []
        for u in range(hdr[5] + hdr[6] * hdr[7]):
            L.check(_lib().mv_gemm_grouped_decode(self.host, u, out), "mv_gemm_grouped_decode")
            res.append(tuple(out))
        return res

    def launch(self, ws=None, accumulate=False, alpha=None):
        L.require_cuda(ws, alpha)
        rc = _lib().mv_gemm_grouped_tn(self.dtype, self.count, self.host, L.ptr(self.dev), L.ptr(ws), (ws.numel() * 4) if ws is not None else 0,
                                       int(accumulate), L.ptr(alpha), L.stream_ptr())
        L.check(rc, f"mv_gemm_grouped_tn(count={self.count})")
        self.launches += 1


def set_gemm_variant(force: int = 0, nj: int = 0):
    L.set_knob("gemm_force", int(force) & 0xff)
    L.set_knob("gemm_nj", int(nj))
    L.set_knob("gemm_dbg", int(force) >> 8)


# ---------------------------------------------------------------------------------------------- report generation (mv_decode.hip)
def gemm_rows(x, w, c, *, M, N, K, ldx=None, ldw=None, ldc=None, bias=None, epi=EPI_NONE, r=None, ldr=None):
    """c[M,N] = epi(x[M,K] . w[N,K]^T) for M <= 256 rows, 16-bit x / w (see mv_gemm_rows); c and r in any of the three encodings."""
    L.require_cuda(x, w, c, bias, r)
    if x.dtype != w.dtype:
        raise TypeError("gemm_rows operands must share a dtype")
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("bias must be f32")
    ldx = ldx if ldx is not None else K
    ldw = ldw if ldw is not None else K
    ldc = ldc if ldc is not None else N
    ldr = ldr if ldr is not None else N
    rc = _lib().mv_gemm_rows(L.dt_of(x), M, N, K, L.ptr(x), ldx, L.ptr(w), ldw, L.ptr(c), ldc, L.dt_of(c), L.ptr(bias), epi, L.ptr(r), ldr,
                             L.dt_of(r) if r is not None else 0, L.stream_ptr())
    L.check(rc, f"mv_gemm_rows(M={M},N={N},K={K},epi={epi})")
    return c


def attn_decode(q, k_cache, v_cache, slots, nk, ctx, *, R, A, dh, max_nk, ldq=None, ldkv=None, ldo=None, slot_row=None, nsplit=0, ws=None):
    """ctx[R, A*dh] = attention of the R query rows over the cache slots each lists (see mv_attn_decode).  slots int32 [rows, ld];
    nk int32 [R]; slot_row int32 [R] or None; ws f32 (split-KV partials) or None."""
    L.require_cuda(q, k_cache, v_cache, slots, nk, ctx, slot_row, ws)
    if slots.dtype != torch.int32 or nk.dtype != torch.int32 or (slot_row is not None and slot_row.dtype != torch.int32):
        raise TypeError("attn_decode: slot tables and counts are int32")
    if not (q.dtype == k_cache.dtype == v_cache.dtype == ctx.dtype):
        raise TypeError("attn_decode: q, caches and ctx share a dtype")
    H = A * dh
    rc = _lib().mv_attn_decode(L.dt_of(q), L.ptr(q), ldq if ldq is not None else H, L.ptr(k_cache), L.ptr(v_cache),
                               ldkv if ldkv is not None else H, L.ptr(slots), slots.shape[-1], L.ptr(slot_row), L.ptr(nk), int(max_nk),
                               L.ptr(ctx), ldo if ldo is not None else H, R, A, dh, int(nsplit), L.ptr(ws),
                               (ws.numel() * 4) if ws is not None else 0, L.stream_ptr())
    L.check(rc, f"mv_attn_decode(R={R},A={A},dh={dh},nsplit={nsplit})")
    return ctx


def logprob_topk(logits, k, *, R=None, V=None, ld=None, eos_penalty_id=-1, vals=None, idx=None, lse=None):
    """(vals f32 [R,k], idx int64 [R,k]) = top-k of log_softmax(logits[:, :V]) with ties to the lower index; eos_penalty_id >= 0 sets
    that column's log-prob to -10000 first (see mv_logprob_topk)."""
    L.require_cuda(logits, vals, idx, lse)
    if logits.dtype != torch.float32:
        raise TypeError("logprob_topk: f32 logits")
    R = R if R is not None else logits.shape[0]
    V = V if V is not None else logits.shape[-1]
    ld = ld if ld is not None else logits.stride(0)
    if vals is None:
        vals = torch.empty((R, k), dtype=torch.float32, device=logits.device)
    if idx is None:
        idx = torch.empty((R, k), dtype=torch.int64, device=logits.device)
    rc = _lib().mv_logprob_topk(L.ptr(logits), ld, R, V, int(k), int(eos_penalty_id), L.ptr(vals), L.ptr(idx), L.ptr(lse), L.stream_ptr())
    L.check(rc, f"mv_logprob_topk(R={R},V={V},k={k})")
    return vals, idx


def ngram_ban(hist_in, hist_out, y, length, n, ban, nban, *, parent=None, ignore=None, R=None):
    """One beam step of n-gram blocking (see mv_ngram_ban): hist_out[r, :length] = hist_in[parent[r], :length], hist_out[r, length] =
    y[r]; ban[r, :nban[r]] = the words that would close a repeated n-gram of the new history, ascending.  hist_* / ban / nban / ignore
    int32, y / parent int64 (parent None: identity).  Nothing is read back."""
    L.require_cuda(hist_in, hist_out, y, ban, nban, parent, ignore)
    if any(t.dtype != torch.int32 for t in (hist_in, hist_out, ban, nban)) or (ignore is not None and ignore.dtype != torch.int32):
        raise TypeError("ngram_ban: histories, ban lists, counts and ignore ids are int32")
    if y.dtype != torch.int64 or (parent is not None and parent.dtype != torch.int64):
        raise TypeError("ngram_ban: y and parent are int64")
    if hist_in.stride(0) != hist_out.stride(0):
        raise ValueError("ngram_ban: the two histories share a leading dimension")
    R = R if R is not None else y.shape[0]
    rc = _lib().mv_ngram_ban(L.ptr(hist_in), L.ptr(hist_out), hist_in.stride(0), L.ptr(parent), L.ptr(y), R, int(length), int(n),
                             L.ptr(ignore), 0 if ignore is None else ignore.numel(), L.ptr(ban), ban.stride(0), L.ptr(nban), L.stream_ptr())
    L.check(rc, f"mv_ngram_ban(R={R},len={length},n={n})")
    return hist_out, ban, nban


def logprob_topk_banned(logits, k, *, R=None, V=None, ld=None, eos_penalty_id=-1, ban=None, nban=None, vals=None, idx=None, lse=None):
    """logprob_topk with -10000 added to the log-prob of every word in ban[r, :nban[r]] (int32) after the normalisation and before the
    EOS rule (see mv_logprob_topk_banned).  ban None: the bits logprob_topk gives."""
    L.require_cuda(logits, vals, idx, lse, ban, nban)
    if logits.dtype != torch.float32:
        raise TypeError("logprob_topk_banned: f32 logits")
    if any(t is not None and t.dtype != torch.int32 for t in (ban, nban)):
        raise TypeError("logprob_topk_banned: ban lists and counts are int32")
    R = R if R is not None else logits.shape[0]
    V = V if V is not None else logits.shape[-1]
    ld = ld if ld is not None else logits.stride(0)
    if vals is None:
        vals = torch.empty((R, k), dtype=torch.float32, device=logits.device)
    if idx is None:
        idx = torch.empty((R, k), dtype=torch.int64, device=logits.device)
    rc = _lib().mv_logprob_topk_banned(L.ptr(logits), ld, R, V, int(k), int(eos_penalty_id), L.ptr(ban), 0 if ban is None else ban.stride(0),
                                       L.ptr(nban), L.ptr(vals), L.ptr(idx), L.ptr(lse), L.stream_ptr())
    L.check(rc, f"mv_logprob_topk_banned(R={R},V={V},k={k})")
    return vals, idx


def embed_rows(ids, pos, seg, E, P, Ty, gamma, beta, out, *, R, H, V, maxpos, eps, ntype=None, ldo=None):
    """out[r] = LN(E[ids[r]] + Ty[seg[r]] + P[pos[r]]) (int64 indices; see mv_embed_rows)."""
    L.require_cuda(ids, pos, seg, E, P, Ty, gamma, beta, out)
    if ids.dtype != torch.int64 or pos.dtype != torch.int64 or seg.dtype != torch.int64:
        raise TypeError("embed_rows: int64 ids / positions / segments")
    rc = _lib().mv_embed_rows(L.dt_of(out), L.ptr(ids), L.ptr(pos), L.ptr(seg), L.ptr(E), L.ptr(P), L.ptr(Ty), L.ptr(gamma), L.ptr(beta),
                              L.ptr(out), ldo if ldo is not None else H, R, H, V, maxpos, ntype if ntype is not None else Ty.shape[0],
                              float(eps), L.stream_ptr())
    L.check(rc, "mv_embed_rows")
    return out


# ---------------------------------------------------------------------------------------------- VQA (mv_vqa.hip)
def bce_fwd_bwd(logits, A, *, R=None, ld=None, target=None, ans_type=None, stats=None, dgrad=None, ldd=None, grad_scale=1.0,
                grad_scale_dev=None, loss_scale_dev=None, arg_train=None, arg_infer=None):
    """BCEWithLogits over soft targets [R, A] (sum into stats[1]), its gradient (padding columns A..ldd zero), the training / inference
    argmax (int64 [R]) and the score split stats f32[6] (see mv_bce_fwd_bwd).  Every output is optional."""
    L.require_cuda(logits, target, ans_type, stats, dgrad, grad_scale_dev, loss_scale_dev, arg_train, arg_infer)
    if logits.dtype != torch.float32 or (target is not None and (target.dtype != torch.float32 or not target.is_contiguous())):
        raise TypeError("bce_fwd_bwd: f32 logits and contiguous f32 targets")
    if ans_type is not None and ans_type.dtype != torch.int32:
        raise TypeError("bce_fwd_bwd: ans_type int32")
    if any(t is not None and t.dtype != torch.int64 for t in (arg_train, arg_infer)):
        raise TypeError("bce_fwd_bwd: argmax outputs int64")
    R = R if R is not None else logits.shape[0]
    ld = ld if ld is not None else logits.stride(0)
    ldd = ldd if ldd is not None else (dgrad.stride(0) if dgrad is not None else 0)
    rc = _lib().mv_bce_fwd_bwd(L.ptr(logits), ld, L.ptr(target), L.ptr(ans_type), R, A, L.ptr(stats), L.ptr(dgrad),
                               L.dt_of(dgrad) if dgrad is not None else 0, ldd, L.ptr(grad_scale_dev), float(grad_scale),
                               L.ptr(loss_scale_dev), L.ptr(arg_train), L.ptr(arg_infer), L.stream_ptr())
    L.check(rc, f"mv_bce_fwd_bwd(R={R},A={A})")


def rows_mul(a, rows_a, b, rows_b, out, *, R, H, lda=None, ldb=None, ldo=None):
    """out[i] = a[rows_a[i]] * b[rows_b[i]] over H columns (int32 row indices; see mv_rows_mul)."""
    L.require_cuda(a, rows_a, b, rows_b, out)
    if not (a.dtype == b.dtype == out.dtype) or rows_a.dtype != torch.int32 or rows_b.dtype != torch.int32:
        raise TypeError("rows_mul: a, b, out share a dtype; int32 row indices")
    rc = _lib().mv_rows_mul(L.dt_of(a), L.ptr(a), lda if lda is not None else H, L.ptr(rows_a), L.ptr(b), ldb if ldb is not None else H,
                            L.ptr(rows_b), R, H, L.ptr(out), ldo if ldo is not None else H, L.stream_ptr())
    L.check(rc, f"mv_rows_mul(R={R},H={H})")
    return out


# ---- BertAdam (csrc/mv_optim.hip) ----
OPTIM_CHUNK = 4096                       # MV_OPTIM_CHUNK of include/medvill.h
SCHEDULE_IDS = {"warmup_linear": 0, "warmup_constant": 1, "warmup_cosine": 2}


def tensor_sqnorms(x, tensors, chunks, partials, out):
    """out[t] = sum of squares of tensor t of the flat f32 buffer x (tables: see mv_tensor_sqnorms; bit-reproducible)."""
    L.require_cuda(x, tensors, chunks, partials, out)
    if x.dtype != torch.float32 or tensors.dtype != torch.int64 or chunks.dtype != torch.int32 or partials.dtype != torch.float32 \
            or out.dtype != torch.float32:
        raise TypeError("tensor_sqnorms: f32 data, int64 tensor table, int32 chunk table")
    T, NC = int(tensors.shape[0]), int(chunks.numel())
    if tensors.dim() != 2 or tensors.shape[1] != 4 or not tensors.is_contiguous() or partials.numel() < NC or out.numel() < T:
        raise ValueError("tensor_sqnorms: tensors [T, 4] contiguous, partials [NC], out [T]")
    rc = _lib().mv_tensor_sqnorms(L.ptr(x), x.numel(), L.ptr(tensors), T, L.ptr(chunks), NC, L.ptr(partials), L.ptr(out), L.stream_ptr())
    L.check(rc, "mv_tensor_sqnorms")
    return out


def bertadam_step(p, g, m, v, tensors, chunks, sqnorms, *, lr, step, warmup=-1.0, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999,
                  eps=1e-6, weight_decay=0.01, max_grad_norm=1.0, shadow=None, shadow_f16=None, scaler_state=None):
    """One BertAdam update of every active tensor of the flat buffers (see mv_bertadam_step); `step` = updates applied before this one."""
    L.require_cuda(p, g, m, v, tensors, chunks, sqnorms, shadow, shadow_f16, scaler_state)
    if any(t.dtype != torch.float32 for t in (p, g, m, v)) or tensors.dtype != torch.int64 or chunks.dtype != torch.int32:
        raise TypeError("bertadam_step: f32 buffers, int64 tensor table, int32 chunk table")
    n = p.numel()
    if any(t.numel() != n for t in (g, m, v)) or any(t is not None and t.numel() != n for t in (shadow, shadow_f16)):
        raise ValueError("bertadam_step: p, g, m, v and the 16-bit copies have one size")
    T, NC = int(tensors.shape[0]), int(chunks.numel())
    if tensors.dim() != 2 or tensors.shape[1] != 4 or not tensors.is_contiguous() or (sqnorms is not None and sqnorms.numel() < T):
        raise ValueError("bertadam_step: tensors [T, 4] contiguous, sqnorms [T]")
    rc = _lib().mv_bertadam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(shadow), L.ptr(shadow_f16), n, L.ptr(tensors), T,
                                 L.ptr(chunks), NC, L.ptr(sqnorms), float(lr), float(b1), float(b2), float(eps), float(weight_decay),
                                 float(max_grad_norm), int(step), int(t_total), float(warmup), SCHEDULE_IDS[schedule],
                                 L.ptr(scaler_state), L.stream_ptr())
    L.check(rc, "mv_bertadam_step")


def bce_multilabel(logits, C, *, R=None, ld=None, target=None, pos_weight=None, loss=None, dgrad=None, ldd=None, grad_scale=1.0,
                   grad_scale_dev=None, loss_scale_dev=None, probs=None, counters=None):
    """BCEWithLogitsLoss(pos_weight) over multi-hot targets [R, C]: loss SUM added to loss[0], gradient (padding columns C..ldd zero),
    sigmoid probabilities [R, C] and the f32 [3, C] {tp, fp, fn} counters (see mv_bce_multilabel).  Every output is optional."""
    L.require_cuda(logits, target, pos_weight, loss, dgrad, grad_scale_dev, loss_scale_dev, probs, counters)
    if logits.dtype != torch.float32 or any(t is not None and (t.dtype != torch.float32 or not t.is_contiguous())
                                            for t in (target, pos_weight, loss, probs, counters)):
        raise TypeError("bce_multilabel: f32 logits; contiguous f32 targets, pos_weight, loss, probs and counters")
    R = R if R is not None else logits.shape[0]
    if (target is not None and target.numel() != R * C) or (pos_weight is not None and pos_weight.numel() != C) \
            or (probs is not None and probs.numel() != R * C) or (counters is not None and counters.numel() != 3 * C):
        raise ValueError("bce_multilabel: target / probs [R, C], pos_weight [C], counters [3, C]")
    ld = ld if ld is not None else logits.stride(0)
    ldd = ldd if ldd is not None else (dgrad.stride(0) if dgrad is not None else 0)
    rc = _lib().mv_bce_multilabel(L.ptr(logits), ld, L.ptr(target), L.ptr(pos_weight), R, C, L.ptr(loss), L.ptr(dgrad),
                                  L.dt_of(dgrad) if dgrad is not None else 0, ldd, L.ptr(grad_scale_dev), float(grad_scale),
                                  L.ptr(loss_scale_dev), L.ptr(probs), L.ptr(counters), L.stream_ptr())
    L.check(rc, f"mv_bce_multilabel(R={R},C={C})")


# ---------------------------------------------------------------------------------------------- report fine-tuning (csrc/mv_lmloss.hip)
def _lm_check(logits, row_ptr, labels, U, V, ld):
    if logits.dtype != torch.float32:
        raise TypeError("lm_loss: f32 logits")
    if row_ptr.dtype != torch.int32 or labels.dtype != torch.int32 or not row_ptr.is_contiguous() or not labels.is_contiguous():
        raise TypeError("lm_loss: contiguous int32 row_ptr and labels")
    if row_ptr.numel() != U + 1 or logits.numel() < (U - 1) * ld + V:
        raise ValueError("lm_loss: row_ptr holds U + 1 offsets and the logits U rows")


def lm_loss_fwd(logits, row_ptr, labels, label_smoothing, *, U=None, V=None, ld=None, entry_loss=None, entry_hit=None, row_stat=None):
    """Per-entry loss of the smoothed masked-LM objective over the CSR entries of the distinct rows (see mv_lm_loss_fwd):
    -> (entry_loss f32 [n], entry_hit int32 [n], row_stat f32 [U, 2])."""
    L.require_cuda(logits, row_ptr, labels, entry_loss, entry_hit, row_stat)
    U = U if U is not None else logits.shape[0]
    V = V if V is not None else logits.shape[-1]
    ld = ld if ld is not None else logits.stride(0)
    n = int(labels.numel())
    _lm_check(logits, row_ptr, labels, U, V, ld)
    dev = logits.device
    entry_loss = entry_loss if entry_loss is not None else torch.empty(n, dtype=torch.float32, device=dev)
    entry_hit = entry_hit if entry_hit is not None else torch.empty(n, dtype=torch.int32, device=dev)
    row_stat = row_stat if row_stat is not None else torch.empty((U, 2), dtype=torch.float32, device=dev)
    if entry_loss.dtype != torch.float32 or entry_hit.dtype != torch.int32 or row_stat.dtype != torch.float32 \
            or entry_loss.numel() < n or entry_hit.numel() < n or row_stat.numel() < 2 * U:
        raise TypeError("lm_loss_fwd: entry_loss f32 [n], entry_hit int32 [n], row_stat f32 [U, 2]")
    rc = _lib().mv_lm_loss_fwd(L.ptr(logits), ld, U, V, L.ptr(row_ptr), L.ptr(labels), n, float(label_smoothing), L.ptr(entry_loss),
                               L.ptr(entry_hit), L.ptr(row_stat), L.stream_ptr())
    L.check(rc, f"mv_lm_loss_fwd(U={U},V={V},n={n})")
    return entry_loss, entry_hit, row_stat


def lm_loss_select(entry_loss, weights, sample, entry_hit, B, k):
    """Drop-worst selection and normalisation (see mv_lm_loss_select): -> (keep int32 [B], stats f32 [4], inv_denom f32 [1])."""
    L.require_cuda(entry_loss, weights, sample, entry_hit)
    n = int(weights.numel())
    if entry_loss.dtype != torch.float32 or weights.dtype != torch.float32 or sample.dtype != torch.int32 \
            or (entry_hit is not None and entry_hit.dtype != torch.int32):
        raise TypeError("lm_loss_select: f32 losses and weights, int32 sample indices and hits")
    if entry_loss.numel() < n or sample.numel() != n or (entry_hit is not None and entry_hit.numel() < n):
        raise ValueError("lm_loss_select: one loss, weight, sample index and hit per entry")
    dev = weights.device
    keep = torch.empty(B, dtype=torch.int32, device=dev)
    stats = torch.empty(4, dtype=torch.float32, device=dev)
    inv = torch.empty(1, dtype=torch.float32, device=dev)
    rc = _lib().mv_lm_loss_select(L.ptr(entry_loss), L.ptr(weights), L.ptr(sample), L.ptr(entry_hit), n, int(B), int(k), L.ptr(keep),
                                  L.ptr(stats), L.ptr(inv), L.stream_ptr())
    L.check(rc, f"mv_lm_loss_select(B={B},k={k},n={n})")
    return keep, stats, inv


def lm_loss_bwd(logits, row_ptr, labels, weights, sample, label_smoothing, row_stat, keep, inv_denom, grad_dev, dlogits, *, U=None,
                V=None, ld=None, ldd=None, loss_scale_dev=None):
    """dlogits [U, ldd] (f32 / bf16 / f16; columns V..ldd-1 zero) of the objective (see mv_lm_loss_bwd)."""
    L.require_cuda(logits, row_ptr, labels, weights, sample, row_stat, keep, inv_denom, grad_dev, dlogits, loss_scale_dev)
    U = U if U is not None else logits.shape[0]
    V = V if V is not None else logits.shape[-1]
    ld = ld if ld is not None else logits.stride(0)
    ldd = ldd if ldd is not None else dlogits.stride(0)
    n = int(labels.numel())
    _lm_check(logits, row_ptr, labels, U, V, ld)
    if weights.dtype != torch.float32 or sample.dtype != torch.int32 or keep.dtype != torch.int32 or weights.numel() != n or sample.numel() != n:
        raise TypeError("lm_loss_bwd: f32 weights [n], int32 sample [n], int32 keep [B]")
    if any(t.dtype != torch.float32 for t in (row_stat, inv_denom, grad_dev)) or row_stat.numel() < 2 * U:
        raise TypeError("lm_loss_bwd: f32 row_stat [U, 2], inv_denom [1], grad_dev [1]")
    if dlogits.numel() < (U - 1) * ldd + max(ldd, V) and U > 0:
        raise ValueError("lm_loss_bwd: dlogits holds U rows of ldd columns")
    rc = _lib().mv_lm_loss_bwd(L.ptr(logits), ld, U, V, L.ptr(row_ptr), L.ptr(labels), L.ptr(weights), L.ptr(sample), n,
                               float(label_smoothing), L.ptr(row_stat), L.ptr(keep), L.ptr(inv_denom), L.ptr(grad_dev),
                               L.ptr(loss_scale_dev), L.ptr(dlogits), L.dt_of(dlogits), ldd, L.stream_ptr())
    L.check(rc, f"mv_lm_loss_bwd(U={U},V={V},n={n})")
    return dlogits


# ---------------------------------------------------------------------------------------------------- retrieval (csrc/mv_retrieval.hip)
RANK_NCOUNT = 28          # mv_rank_groups' counters: include/medvill.h
PAIR_MAX_DRAWS = 300


def _words_to_i32(w):
    """32-bit words given as integers in [0, 2^32) (any integer dtype) -> their bit patterns in an int32 tensor."""
    w = torch.as_tensor(w).to(torch.int64)
    return (((w + 2 ** 31) % 2 ** 32) - 2 ** 31).to(torch.int32)


def _i32_to_words(w):
    return w.to(torch.int64) & 0xFFFFFFFF


def pair_draws(key, step, B, D, device):
    """int64 [B, D, 2] holding the 32-bit words {w0, w1} of attempt t of sample i (see mv_pair_draws)."""
    out = torch.empty((B, D, 2), dtype=torch.int32, device=device)
    L.require_cuda(out)
    rc = _lib().mv_pair_draws(int(key) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(B), int(D), L.ptr(out), L.stream_ptr())
    L.check(rc, f"mv_pair_draws(B={B},D={D})")
    return _i32_to_words(out)


def pair_negatives(idx, n, key=0, step=0, class_id=None, draws=None):
    """The retrieval training sampler (see mv_pair_negatives): idx int32 [B] on the device -> (pairs int32 [2B, 2], labels int32 [2B]).
    draws: integers in [0, 2^32), [B, D, 2] (or [B, 2] for D = 1), replacing the hash-generated words."""
    L.require_cuda(idx, class_id)
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise TypeError("pair_negatives: idx int32 [B]")
    if class_id is not None and (class_id.dtype != torch.int32 or tuple(class_id.shape) != (int(n),)):
        raise TypeError("pair_negatives: class_id int32 [n]")
    B, dev = int(idx.numel()), idx.device
    d32, D = None, 0
    if draws is not None:
        d32 = _words_to_i32(draws).to(dev).reshape(B, -1, 2).contiguous()
        D = int(d32.shape[1])
    pairs = torch.empty((2 * B, 2), dtype=torch.int32, device=dev)
    labels = torch.empty((2 * B,), dtype=torch.int32, device=dev)
    rc = _lib().mv_pair_negatives(L.ptr(idx.contiguous()), B, int(n), L.ptr(class_id), int(key) & 0xFFFFFFFFFFFFFFFF,
                                  int(step) & 0xFFFFFFFFFFFFFFFF, L.ptr(d32), D, L.ptr(pairs), L.ptr(labels), L.stream_ptr())
    L.check(rc, f"mv_pair_negatives(B={B},n={n})")
    return pairs, labels


def _bank_check(who, txt_ids, txt_len, img_feats, img_pos, idx, family=None, per_text=(), pairs=False):
    """What the four *_assemble wrappers check alike: -> (text rows, T, images, N, F, samples).  idx: the int32 index list [B], or
    (pairs) the [R, 2] (image item, text item) list; per_text: further int32 tensors with one entry per text row; img_pos: None where
    the caller allows a bank without positions.  (These run once per batch next to a 25 us kernel: plain loops, no generators.)"""
    i32 = (txt_len, idx, *per_text) if family is None else (txt_len, idx, family, *per_text)
    L.require_cuda(txt_ids, img_feats, img_pos, *i32)
    if txt_ids.dtype != torch.int64 or (img_pos is not None and img_pos.dtype != torch.int64) or [t for t in i32 if t.dtype != torch.int32]:
        raise TypeError(f"{who}: txt_ids / img_pos int64, every length, index and family tensor int32")
    if txt_ids.dim() != 2 or img_feats.dim() != 3 or idx.dim() != (2 if pairs else 1) or (pairs and idx.shape[1] != 2):
        raise ValueError(f"{who}: txt_ids [text rows, T], img_feats [images, N, F], {'pairs [R, 2]' if pairs else 'idx [B]'}")
    n, T = txt_ids.shape
    n_img, N, F = img_feats.shape
    B = idx.shape[0]
    if txt_len.shape != (n,) or [t for t in per_text if t.shape != (n,)] or (img_pos is not None and img_pos.shape != (n_img, N)) \
            or (family is not None and family.shape != (B,)):
        raise ValueError(f"{who}: one entry per text row, one position row per image, one family per sample")
    if not (txt_ids.is_contiguous() and img_feats.is_contiguous() and (img_pos is None or img_pos.is_contiguous())) \
            or [t for t in i32 if not t.is_contiguous()]:
        raise ValueError(f"{who}: contiguous tensors")
    return n, T, n_img, N, F, B


def _bank_outputs(B, T, N, F, img_feats, pos=True):
    """The outputs every assemble kernel writes; the caller adds its own."""
    dev = img_feats.device
    return dict(input_txt=torch.empty((B, T), dtype=torch.int64, device=dev), segment=torch.empty((B, T), dtype=torch.int64, device=dev),
                desc=torch.empty((B, 3), dtype=torch.int32, device=dev), feats=torch.empty((B, N, F), dtype=img_feats.dtype, device=dev),
                pos=torch.empty((B, N), dtype=torch.int64, device=dev) if pos else None)


def pair_assemble(txt_ids, txt_len, img_feats, img_pos, pairs):
    """Pair batches from the banks (see mv_pair_assemble): -> dict(input_txt, segment, n_ids, desc, feats, pos)."""
    Ti, T, Ii, N, F, R = _bank_check("pair_assemble", txt_ids, txt_len, img_feats, img_pos, pairs, pairs=True)
    out = _bank_outputs(R, T, N, F, img_feats, pos=img_pos is not None)
    out["n_ids"] = torch.empty((R,), dtype=torch.int32, device=pairs.device)
    rc = _lib().mv_pair_assemble(L.ptr(txt_ids), L.ptr(txt_len), Ti, L.ptr(img_feats), L.dt_of(img_feats), Ii, L.ptr(img_pos),
                                 L.ptr(pairs), R, N, T - 1, F, L.ptr(out["input_txt"]), L.ptr(out["segment"]),
                                 L.ptr(out["n_ids"]), L.ptr(out["desc"]), L.ptr(out["feats"]), L.ptr(out["pos"]), L.stream_ptr())
    if rc:
        L.check(rc, f"mv_pair_assemble(R={R},N={N},S={T - 1},F={F})")
    return out


def rank_groups(logits, labels, C, ks=(1, 5, 10), counters=None):
    """Ranking of G groups of C candidates (see mv_rank_groups): -> (p f32 [G*C], pos int32 [G*C], rank int32 [G], counters int64 [28]);
    `counters` (int64 [28] on the device) is accumulated into when given."""
    import ctypes
    L.require_cuda(logits, labels, counters)
    if logits.dtype != torch.float32 or labels.dtype != torch.int32 or not logits.is_contiguous() or not labels.is_contiguous():
        raise TypeError("rank_groups: contiguous f32 logits [G*C, 2] and int32 labels [G*C]")
    n, C = int(labels.numel()), int(C)
    if C < 1 or n == 0 or n % C != 0 or logits.numel() != 2 * n:
        raise ValueError(f"rank_groups: {n} candidates do not form groups of {C} (logits [G*C, 2], labels [G*C])")
    dev = logits.device
    if counters is None:
        counters = torch.zeros(RANK_NCOUNT, dtype=torch.int64, device=dev)
    elif counters.dtype != torch.int64 or counters.numel() != RANK_NCOUNT or not counters.is_contiguous():
        raise TypeError(f"rank_groups: counters int64 [{RANK_NCOUNT}]")
    ks = [int(k) for k in ks]
    karr = (ctypes.c_int * max(len(ks), 1))(*ks)
    p = torch.empty(n, dtype=torch.float32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    rank = torch.empty(n // C, dtype=torch.int32, device=dev)
    rc = _lib().mv_rank_groups(L.ptr(logits), L.ptr(labels), n // C, C, ctypes.cast(karr, ctypes.c_void_p), len(ks), L.ptr(p), L.ptr(pos),
                               L.ptr(rank), L.ptr(counters), L.stream_ptr())
    L.check(rc, f"mv_rank_groups(G={n // C},C={C},ks={ks})")
    return p, pos, rank, counters


# ---------------------------------------------------------------------------------------------------- report bank (csrc/mv_report.hip)
def report_draws(key, step, B, T, device):
    """int64 [B, T+1] holding the 32-bit words of the masking draw (see mv_report_draws): T shuffle keys and the coin per sample."""
    out = torch.empty((B, T + 1), dtype=torch.int32, device=device)
    L.require_cuda(out)
    rc = _lib().mv_report_draws(int(key) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(B), int(T), L.ptr(out), L.stream_ptr())
    L.check(rc, f"mv_report_draws(B={B},T={T})")
    return _i32_to_words(out)


def report_assemble(txt_ids, txt_len, n_pred, img_feats, img_pos, idx, max_pred, family=None, key=0, step=0, draws=None):
    """Report fine-tuning batches from the banks (see mv_report_assemble): -> dict(input_txt, segment, desc, feats, pos, masked_pos,
    masked_lm_labels, masked_weights).  draws: integers in [0, 2^32), [B, T+1], replacing the hash-generated words."""
    n, T, n_img, N, F, B = _bank_check("report_assemble", txt_ids, txt_len, img_feats, img_pos, idx, family, per_text=(n_pred,))
    if n_img != n:
        raise ValueError("report_assemble: one image per item")
    d32 = None
    if draws is not None:
        d32 = _words_to_i32(draws).to(txt_ids.device).contiguous()
        if tuple(d32.shape) != (B, T + 1):
            raise ValueError(f"report_assemble: draws [B, T+1] = [{B}, {T + 1}]")
    P = int(max_pred)
    out = _bank_outputs(B, T, N, F, img_feats)
    for k, dt in (("masked_pos", torch.int64), ("masked_lm_labels", torch.int64), ("masked_weights", torch.float32)):
        out[k] = torch.empty((B, P), dtype=dt, device=idx.device)
    rc = _lib().mv_report_assemble(L.ptr(txt_ids), L.ptr(txt_len), L.ptr(n_pred), n, L.ptr(img_feats), L.dt_of(img_feats), L.ptr(img_pos),
                                   L.ptr(idx), L.ptr(family), B, N, T, F, P, int(key) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                   L.ptr(d32), L.ptr(out["input_txt"]), L.ptr(out["segment"]), L.ptr(out["desc"]), L.ptr(out["feats"]),
                                   L.ptr(out["pos"]), L.ptr(out["masked_pos"]), L.ptr(out["masked_lm_labels"]),
                                   L.ptr(out["masked_weights"]), L.stream_ptr())
    if rc:
        L.check(rc, f"mv_report_assemble(B={B},N={N},T={T},F={F},max_pred={P})")
    return out


def report_plan(masked_pos, masked_lm_labels, masked_weights, L_seq, V, valid_len=None):
    """report_finetune.build_plan on the device (see mv_report_plan): int64 [B, P] positions and labels, f32 [B, P] weights ->
    dict(rows, row_ptr, labels, weights, sample, counts): full-size buffers (B P elements, row_ptr one more) of which the first
    counts[0] rows / counts[1] entries are written; counts int32 [4] = {U, n, bad, 0}.  Nothing is read back here."""
    L.require_cuda(masked_pos, masked_lm_labels, masked_weights, valid_len)
    if masked_pos.dtype != torch.int64 or masked_lm_labels.dtype != torch.int64 or masked_weights.dtype != torch.float32 \
            or (valid_len is not None and valid_len.dtype != torch.int32):
        raise TypeError("report_plan: int64 positions and labels, f32 weights, int32 valid_len")
    if masked_pos.dim() != 2 or masked_pos.shape != masked_lm_labels.shape or masked_pos.shape != masked_weights.shape:
        raise ValueError("report_plan: positions, labels and weights share one [B, max_pred] shape")
    B, P = (int(s) for s in masked_pos.shape)
    if valid_len is not None and (valid_len.numel() != B or not valid_len.is_contiguous()):
        raise ValueError("report_plan: valid_len [B]")
    if not (masked_pos.is_contiguous() and masked_lm_labels.is_contiguous() and masked_weights.is_contiguous()):
        raise ValueError("report_plan: contiguous tensors")
    dev = masked_pos.device
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    out = dict(rows=i32(B * P), row_ptr=i32(B * P + 1), labels=i32(B * P), weights=torch.empty(B * P, dtype=torch.float32, device=dev),
               sample=i32(B * P), counts=i32(4))
    work = i32(3 * B)
    rc = _lib().mv_report_plan(L.ptr(masked_pos), L.ptr(masked_lm_labels), L.ptr(masked_weights), L.ptr(valid_len), B, P, int(L_seq), int(V),
                               L.ptr(work), L.ptr(out["rows"]), L.ptr(out["row_ptr"]), L.ptr(out["labels"]), L.ptr(out["weights"]),
                               L.ptr(out["sample"]), L.ptr(out["counts"]), L.stream_ptr())
    L.check(rc, f"mv_report_plan(B={B},P={P},L={L_seq},V={V})")
    return out


# ---------------------------------------------------------------------------------------------------- VQA bank (csrc/mv_vqa_bank.hip)
VQA_MAX_GROUPS = 8        # mv_vqa_score's counters: uint64 [G, 3, 2], G <= 8 (include/medvill.h)


def _vqa_csr_check(who, n, ans_ptr, ans_label, ans_score, ans_type):
    if ans_ptr.dtype != torch.int32 or ans_label.dtype != torch.int32 or ans_score.dtype != torch.float32 or ans_type.dtype != torch.int32:
        raise TypeError(f"{who}: ans_ptr / ans_label / ans_type int32, ans_score f32")
    if tuple(ans_ptr.shape) != (n + 1,) or tuple(ans_type.shape) != (n,) or ans_label.dim() != 1 or ans_label.shape != ans_score.shape:
        raise ValueError(f"{who}: ans_ptr [n+1], ans_label / ans_score [nnz], ans_type [n]")
    if not all(t.is_contiguous() for t in (ans_ptr, ans_label, ans_score, ans_type)):
        raise ValueError(f"{who}: contiguous tensors")
    return int(ans_label.numel())


def vqa_assemble(txt_ids, txt_len, q_img, ans_ptr, ans_label, ans_score, ans_type, img_feats, img_pos, idx, n_answers, family=None):
    """VQA batches from the question bank (see mv_vqa_assemble): -> dict(input_txt, segment, desc, feats, pos, target, ans_type)."""
    L.require_cuda(ans_ptr, ans_label, ans_score, ans_type)
    n, T, n_img, N, F, B = _bank_check("vqa_assemble", txt_ids, txt_len, img_feats, img_pos, idx, family, per_text=(q_img,))
    nnz, A = _vqa_csr_check("vqa_assemble", n, ans_ptr, ans_label, ans_score, ans_type), int(n_answers)
    out = _bank_outputs(B, T, N, F, img_feats)
    out["target"] = torch.empty((B, A), dtype=torch.float32, device=idx.device)
    out["ans_type"] = torch.empty((B,), dtype=torch.int32, device=idx.device)
    rc = _lib().mv_vqa_assemble(L.ptr(txt_ids), L.ptr(txt_len), L.ptr(q_img), n, L.ptr(ans_ptr), L.ptr(ans_label) or None,
                                L.ptr(ans_score) or None, nnz, L.ptr(ans_type), L.ptr(img_feats), L.dt_of(img_feats), L.ptr(img_pos), n_img,
                                L.ptr(idx), L.ptr(family), B, N, T, F, A, L.ptr(out["input_txt"]), L.ptr(out["segment"]), L.ptr(out["desc"]),
                                L.ptr(out["feats"]), L.ptr(out["pos"]), L.ptr(out["target"]), L.ptr(out["ans_type"]), L.stream_ptr())
    if rc:
        L.check(rc, f"mv_vqa_assemble(B={B},N={N},T={T},F={F},A={A})")
    return out


def vqa_score(pred, idx, ans_ptr, ans_label, ans_score, ans_type, group=None, G=VQA_MAX_GROUPS, counters=None, want_score=True):
    """The score of predicted answer columns against the bank's sparse answers (see mv_vqa_score): pred int64 [B], idx int32 [B] ->
    (score f32 [B] or None, counters int64 [G, 3, 2] = {sum of fx(score), samples} by group and type slot closed / open / neither);
    `counters` (on the device) is accumulated into when given."""
    L.require_cuda(pred, idx, ans_ptr, ans_label, ans_score, ans_type, group, counters)
    if pred.dtype != torch.int64 or idx.dtype != torch.int32 or (group is not None and group.dtype != torch.int32):
        raise TypeError("vqa_score: pred int64, idx / group int32")
    B, n, G = int(pred.numel()), int(ans_type.numel()), int(G)
    if pred.dim() != 1 or tuple(idx.shape) != (B,) or not pred.is_contiguous() or not idx.is_contiguous():
        raise ValueError("vqa_score: contiguous pred [B] and idx [B]")
    nnz = _vqa_csr_check("vqa_score", n, ans_ptr, ans_label, ans_score, ans_type)
    if group is not None and (tuple(group.shape) != (n,) or not group.is_contiguous()):
        raise ValueError("vqa_score: group [n_questions]")
    dev = pred.device
    if counters is None:
        counters = torch.zeros((max(G, 1), 3, 2), dtype=torch.int64, device=dev)
    elif counters.dtype != torch.int64 or counters.numel() != G * 6 or not counters.is_contiguous():
        raise TypeError(f"vqa_score: counters int64 [{G}, 3, 2]")
    score = torch.empty(B, dtype=torch.float32, device=dev) if want_score else None
    rc = _lib().mv_vqa_score(L.ptr(pred), L.ptr(idx), B, n, L.ptr(ans_ptr), L.ptr(ans_label) or None, L.ptr(ans_score) or None, nnz,
                             L.ptr(ans_type), L.ptr(group), G, L.ptr(score), L.ptr(counters), L.stream_ptr())
    L.check(rc, f"mv_vqa_score(B={B},G={G})")
    return score, counters


# ---------------------------------------------------------------------------------------------------- classification bank (csrc/mv_clf_bank.hip)
CLF_MAX_CLASSES = 1024          # mv_clf_assemble / mv_clf_counts: C <= 1024 (include/medvill.h)
CLF_MAX_ELEMS = 1 << 21         # mv_clf_counts: n C <= 2^21 (pair counting is quadratic)
CLF_NCOUNT = 7                  # n_pos, n_neg, gt, eq, tp, fp, fn


def _clf_bits_check(who, lab_bits, C):
    L.require_cuda(lab_bits)
    if lab_bits.dtype != torch.int32 or lab_bits.dim() != 2 or lab_bits.shape[1] != (C + 31) // 32 or not lab_bits.is_contiguous():
        raise TypeError(f"{who}: lab_bits contiguous int32 [samples, ceil(C / 32)]")
    return int(lab_bits.shape[0])


def clf_assemble(txt_ids, txt_len, s_img, lab_bits, img_feats, img_pos, idx, n_classes, family=None):
    """Classification batches from the sample bank (see mv_clf_assemble): -> dict(input_txt, segment, desc, feats, pos, target)."""
    C = int(n_classes)
    n, T, n_img, N, F, B = _bank_check("clf_assemble", txt_ids, txt_len, img_feats, img_pos, idx, family, per_text=(s_img,))
    if _clf_bits_check("clf_assemble", lab_bits, C) != n:
        raise ValueError("clf_assemble: one row of label bits per text row")
    out = _bank_outputs(B, T, N, F, img_feats)
    out["target"] = torch.empty((B, C), dtype=torch.float32, device=idx.device)
    rc = _lib().mv_clf_assemble(L.ptr(txt_ids), L.ptr(txt_len), L.ptr(s_img), L.ptr(lab_bits), n, L.ptr(img_feats), L.dt_of(img_feats),
                                L.ptr(img_pos), n_img, L.ptr(idx), L.ptr(family), B, N, T, F, C, L.ptr(out["input_txt"]),
                                L.ptr(out["segment"]), L.ptr(out["desc"]), L.ptr(out["feats"]), L.ptr(out["pos"]), L.ptr(out["target"]),
                                L.stream_ptr())
    if rc:
        L.check(rc, f"mv_clf_assemble(B={B},N={N},T={T},F={F},C={C})")
    return out


def clf_counts(probs, idx, lab_bits, n_classes, counters=None):
    """The integer counts of an evaluation (see mv_clf_counts): probs f32 [n, ld >= C] (rows may be strided), idx int32 [n] ->
    counters int64 [C + 1, 7] = {n_pos, n_neg, gt, eq, tp, fp, fn} per class and, in row C, over all n C elements as one list;
    `counters` (on the device) is accumulated into when given."""
    C = int(n_classes)
    L.require_cuda(probs, idx, counters)
    if probs.dtype != torch.float32 or idx.dtype != torch.int32:
        raise TypeError("clf_counts: probs f32, idx int32")
    if probs.dim() != 2 or probs.shape[1] < C or probs.stride(1) != 1 or probs.stride(0) < probs.shape[1] or idx.dim() != 1 \
            or idx.shape[0] != probs.shape[0] or not idx.is_contiguous():
        raise ValueError("clf_counts: probs [n, >= C] with unit column stride and contiguous idx [n]")
    n_items, n = _clf_bits_check("clf_counts", lab_bits, C), int(probs.shape[0])
    if counters is None:
        counters = torch.zeros((C + 1, CLF_NCOUNT), dtype=torch.int64, device=probs.device)
    elif counters.dtype != torch.int64 or counters.numel() != (C + 1) * CLF_NCOUNT or not counters.is_contiguous():
        raise TypeError(f"clf_counts: counters int64 [{C + 1}, {CLF_NCOUNT}]")
    rc = _lib().mv_clf_counts(L.ptr(probs), int(probs.stride(0)), L.ptr(idx), n, L.ptr(lab_bits), n_items, C, L.ptr(counters),
                              L.stream_ptr())
    L.check(rc, f"mv_clf_counts(n={n},C={C})")
    return counters


# ---------------------------------------------------------------------------------------------------- corpus BLEU (csrc/mv_bleu.hip)
BLEU_MAX_WORDS = 1024           # mv_bleu_words / mv_bleu_counts: tokens or words per row (include/medvill.h)
BLEU_MAX_VOCAB = 1 << 20
BLEU_MAX_ROWS = 1 << 20
BLEU_NCOUNT = 10                # num_1..4, den_1..4, hyp_len, ref_len


def _bleu_rows(who, key, cnt):
    if key.dtype != torch.int64 or cnt.dtype != torch.int32:
        raise TypeError(f"{who}: word keys int64, word counts int32")
    if key.dim() != 2 or not key.is_contiguous() or cnt.dim() != 1 or cnt.shape[0] != key.shape[0] or not cnt.is_contiguous():
        raise ValueError(f"{who}: contiguous word keys [rows, words] and one count per row")


def bleu_words(ids, tok_key, tail_key, tail_pow, eos_id, pad_id, empty_key):
    """The word keys of generated rows (see mv_bleu_words): ids int64 [n, T] (rows may be strided), the three int64 [V] tables of
    report_eval.word_tables -> (word_key int64 [n, T], n_words int32 [n])."""
    L.require_cuda(ids, tok_key, tail_key, tail_pow)
    tables = (tok_key, tail_key, tail_pow)
    if ids.dtype != torch.int64 or any(t.dtype != torch.int64 for t in tables):
        raise TypeError("bleu_words: ids and the tables are int64")
    if ids.dim() != 2 or ids.stride(1) != 1 or ids.stride(0) < ids.shape[1]:
        raise ValueError("bleu_words: ids [n, T] with unit column stride")
    V = int(tok_key.numel())
    if any(t.dim() != 1 or t.numel() != V or not t.is_contiguous() for t in tables):
        raise ValueError("bleu_words: three contiguous tables over one vocabulary")
    n, T = int(ids.shape[0]), int(ids.shape[1])
    word_key = torch.empty((n, T), dtype=torch.int64, device=ids.device)
    n_words = torch.empty(n, dtype=torch.int32, device=ids.device)
    rc = _lib().mv_bleu_words(L.ptr(ids), int(ids.stride(0)), n, T, L.ptr(tok_key), L.ptr(tail_key), L.ptr(tail_pow), V, int(eos_id),
                              int(pad_id), int(empty_key), L.ptr(word_key), L.ptr(n_words), L.stream_ptr())
    L.check(rc, f"mv_bleu_words(n={n},T={T},V={V})")
    return word_key, n_words


def bleu_counts(hyp_key, hyp_n, ref_key, ref_n, idx, counters=None):
    """The integer counts corpus BLEU-1..4 follow from (see mv_bleu_counts): hypothesis rows [n, Th] / [n], reference rows
    [n_items, Tr] / [n_items], idx int32 [n] -> counters int64 [10] = {num_1..4, den_1..4, hyp_len, ref_len}; `counters` (on the
    device) is accumulated into when given."""
    L.require_cuda(hyp_key, hyp_n, ref_key, ref_n, idx, counters)
    _bleu_rows("bleu_counts", hyp_key, hyp_n)
    _bleu_rows("bleu_counts", ref_key, ref_n)
    n = int(hyp_key.shape[0])
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.shape[0] != n or not idx.is_contiguous():
        raise TypeError("bleu_counts: idx contiguous int32, one per hypothesis row")
    if counters is None:
        counters = torch.zeros(BLEU_NCOUNT, dtype=torch.int64, device=hyp_key.device)
    elif counters.dtype != torch.int64 or counters.numel() != BLEU_NCOUNT or not counters.is_contiguous():
        raise TypeError(f"bleu_counts: counters int64 [{BLEU_NCOUNT}]")
    rc = _lib().mv_bleu_counts(L.ptr(hyp_key), int(hyp_key.shape[1]), L.ptr(hyp_n), n, L.ptr(ref_key), int(ref_key.shape[1]), L.ptr(ref_n),
                               int(ref_key.shape[0]), L.ptr(idx), L.ptr(counters), L.stream_ptr())
    L.check(rc, f"mv_bleu_counts(n={n})")
    return counters
