"""CPU-reachable half of the C ABI: every entry point validates its arguments BEFORE it touches the HIP runtime, so the rejections
(null pointers, shapes and alignments the kernels do not support, dtype codes, workspaces that are too small) and the one HOST
function (mv_mask_verify_host) can be exercised without a GPU -- also under AddressSanitizer / UBSan (tools/asan_host_check.sh
builds the library's host side with -fsanitize=address,undefined and runs this file and tests/test_abi.py against it)."""
import ctypes as C

import numpy as np
import pytest

import medvill_amd  # noqa: F401
from medvill_amd import _lib

E_ARG, E_SHAPE, E_DTYPE, E_WS = -1, -2, -3, -4
F32, BF16, F16 = 0, 1, 2
P = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below must return before a launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def gemm(lib, dtype=BF16, ta=0, tb=0, M=64, N=64, K=64, A=P, lda=64, B=P, ldb=64, Cp=P, ldc=64, c_dtype=BF16, bias=None, epi=0, R=None,
         ldr=64, r_dtype=BF16, C2=None, ldc2=64, C3=None, ldc3=64, c3_dtype=BF16, splitk=1, ws=None, ws_bytes=0, accumulate=0,
         alpha=None, cpart=None):
    return lib.mv_gemm(dtype, ta, tb, M, N, K, A, lda, B, ldb, Cp, ldc, c_dtype, bias, epi, R, ldr, r_dtype, C2, ldc2, C3, ldc3, c3_dtype,
                       splitk, ws, ws_bytes, accumulate, 0.0, 0, alpha, cpart, None)


def test_gemm_rejects(lib):
    assert gemm(lib, A=None) == E_ARG and gemm(lib, B=None) == E_ARG and gemm(lib, Cp=None) == E_ARG
    assert gemm(lib, M=0) == E_ARG and gemm(lib, K=-3) == E_ARG
    assert gemm(lib, dtype=7) == E_DTYPE and gemm(lib, c_dtype=-1) == E_DTYPE
    assert gemm(lib, C3=P, c3_dtype=F32) == E_DTYPE and gemm(lib, C3=P, ldc3=8) == E_DTYPE
    assert gemm(lib, epi=11) == E_ARG and gemm(lib, epi=-1) == E_ARG
    for epi in (1, 2, 3, 6, 7, 9, 10):
        assert gemm(lib, epi=epi) == E_ARG                     # bias missing
    for epi in (3, 4, 5, 8, 10):
        assert gemm(lib, epi=epi, bias=P) == E_ARG             # elementwise operand missing
    assert gemm(lib, epi=5, R=P, r_dtype=9) == E_ARG
    assert gemm(lib, epi=2, bias=P) == E_ARG and gemm(lib, epi=7, bias=P) == E_ARG          # second output missing
    assert gemm(lib, lda=8) == E_SHAPE and gemm(lib, ldb=8) == E_SHAPE and gemm(lib, ldc=8) == E_SHAPE
    assert gemm(lib, ta=1, M=128, lda=64) == E_SHAPE and gemm(lib, tb=1, N=128, ldb=64, ldc=128) == E_SHAPE
    assert gemm(lib, epi=5, R=P, ldr=8) == E_SHAPE
    assert gemm(lib, splitk=4, c_dtype=F32, epi=1, bias=P) == E_SHAPE and gemm(lib, splitk=4) == E_SHAPE       # split-K: plain f32 output only
    assert gemm(lib, accumulate=1) == E_SHAPE
    assert gemm(lib, splitk=4, c_dtype=F32) == E_WS
    assert gemm(lib, splitk=4, c_dtype=F32, ws=P, ws_bytes=4 * 64 * 64 * 4 - 1) == E_WS
    assert gemm(lib, alpha=P) == E_ARG                         # alpha: f32 output without an epilogue only


def test_mask_and_plan_rejects(lib):
    assert lib.mv_mask_pack(None, 3, 2, 64, P, P, None) == E_ARG and lib.mv_mask_pack(P, 3, 0, 64, P, P, None) == E_ARG
    assert lib.mv_mask_pack(P, 4, 2, 64, P, P, None) == E_SHAPE and lib.mv_mask_pack(P, 1, 2, 64, P, P, None) == E_SHAPE      # NotImplementedError
    assert lib.mv_mask_pack(P, 3, 2, 64 * 64 + 1, P, P, None) == E_SHAPE
    assert lib.mv_mask_build(None, 2, 64, P, P, None) == E_ARG and lib.mv_mask_build(P, 2, 0, P, P, None) == E_ARG
    assert lib.mv_mask_build(P, 2, 5000, P, P, None) == E_SHAPE
    assert lib.mv_pack_plan(None, 2, 64, P, P, P, None) != 0
    assert lib.mv_tail_perm(None, 2, 64, P, 4, P, P, P, P, None) != 0


def test_attention_rejects(lib):
    fwd = lambda **k: lib.mv_attn_fwd(k.get("dt", BF16), k.get("qkv", P), P, P, k.get("ctx", P), k.get("ctx2", None), P, k.get("B", 2),
                                      k.get("L", 64), 2, k.get("dh", 64), k.get("p", 0.0), k.get("db", None), k.get("cu", None),
                                      k.get("rows", 0), None, None)
    assert fwd(qkv=None) == E_ARG and fwd(B=0) == E_ARG and fwd(dh=0) == E_ARG
    assert fwd(dt=5) == E_DTYPE and fwd(dt=BF16, ctx2=P) == E_DTYPE
    assert fwd(dh=32) == E_SHAPE                               # the MFMA kernels are built for dh = 64
    assert fwd(qkv=P + 4) == E_SHAPE                           # 16-byte alignment of the fused projection
    assert fwd(cu=P, rows=0) == E_ARG and fwd(cu=P, rows=2 * 64 + 1) == E_ARG
    assert fwd(p=0.1) != 0                                     # dropout needs the keep-bit tensor
    assert lib.mv_attn_bwd(BF16, None, P, P, P, P, P, P, P, 2, 64, 2, 64, 0.0, None, None, 0, None, None) == E_ARG
    assert lib.mv_attn_dropmask(0.1, 1, 2, 64, 2, None, None, None) == E_ARG


def test_attention_entry_points_reject_before_any_launch(lib):
    """Every reject path of mv_attn_fwd / mv_attn_bwd / mv_attn_dropmask / mv_mask_pack / mv_mask_build.  The outputs are real, NaN-filled
    host buffers, compared afterwards: the host side of a launcher that returns an error has written nothing.  (That nothing was
    launched is the error code's word, as everywhere in this file: a kernel could not write host memory anyway.)  mv_attn_bwd does not
    check the alignment of ctx (include/medvill.h says why), so that reject exists for the forward only."""
    def aligned(n, dt, fill):                # 64-byte aligned, whatever the allocator returns
        raw = np.empty(n * np.dtype(dt).itemsize + 64, dtype=np.uint8)
        a = raw[(-raw.ctypes.data) % 64:][:n * np.dtype(dt).itemsize].view(dt)
        a[...] = fill
        return a
    nan = lambda n, dt=np.float32: aligned(n, dt, np.nan)
    B, L, A = 2, 64, 2
    ctx, ctx2, lse, dqkv, delta = nan(B * L * A * 64, np.float16), nan(B * L * A * 64, np.float16), nan(B * A * L), nan(B * L * 3 * A * 64, np.float16), nan(B * A * L)
    bits, info, db = aligned(B * L * 2, np.uint32, 0x5A5A5A5A), aligned(B, np.uint8, 0xA5), aligned(B * A * 2 * 64, np.uint32, 0x3C3C3C3C)
    outs = (ctx, ctx2, lse, dqkv, delta, bits, info, db)
    before = [o.copy() for o in outs]
    ptr = lambda a: a.ctypes.data
    assert all(ptr(o) % 16 == 0 for o in (ctx, ctx2, dqkv)) and ptr(db) % 64 == 0

    def fwd(dt=BF16, qkv=P, bits_=P, info_=P, ctx_=None, ctx2_=None, lse_=None, B_=B, L_=L, A_=A, dh=64, p=0.0, db_=None, cu=None, rows=0, qlim=None):
        return lib.mv_attn_fwd(dt, qkv, bits_, info_, ptr(ctx) if ctx_ is None else ctx_, ctx2_, ptr(lse) if lse_ is None else lse_, B_, L_, A_, dh, p,
                               db_, cu, rows, qlim, None)

    def bwd(dt=BF16, qkv=P, ctx_=P, dctx=P, lse_=P, bits_=P, info_=P, dqkv_=None, delta_=None, B_=B, L_=L, A_=A, dh=64, p=0.0, db_=None, cu=None,
            rows=0, qlim=None):
        return lib.mv_attn_bwd(dt, qkv, ctx_, dctx, lse_, bits_, info_, ptr(dqkv) if dqkv_ is None else dqkv_, ptr(delta) if delta_ is None else delta_,
                               B_, L_, A_, dh, p, db_, cu, rows, qlim, None)

    for f in (fwd, bwd):
        # 16-bit MFMA path
        for dt in (BF16, F16):
            assert f(dt=dt, dh=32) == E_SHAPE and f(dt=dt, dh=128) == E_SHAPE and f(dt=dt, dh=65) == E_SHAPE
            assert f(dt=dt, cu=P, rows=0) == E_ARG and f(dt=dt, cu=P, rows=-1) == E_ARG and f(dt=dt, cu=P, rows=B * L + 1) == E_ARG
            assert f(dt=dt, qkv=P + 8) == E_SHAPE and f(dt=dt, qkv=P + 2) == E_SHAPE
        # dropout arguments
        assert f(p=1.0, db_=ptr(db)) == E_ARG and f(p=1.5, db_=ptr(db)) == E_ARG and f(p=0.1) == E_ARG and f(dt=F32, p=0.1) == E_ARG
        assert f(p=0.1, db_=ptr(db) + 32) == E_SHAPE and f(p=0.1, db_=ptr(db) + 4) == E_SHAPE
        # encoding and path limits
        assert f(dt=F32, cu=P, rows=B * L) == E_SHAPE and f(dt=F32, qlim=P) == E_SHAPE and f(dt=F32, dh=129) == E_SHAPE and f(dt=F32, dh=256) == E_SHAPE
        assert f(dt=3) == E_DTYPE and f(dt=-1) == E_DTYPE
        # null pointers and non-positive sizes
        assert f(qkv=None) == E_ARG and f(bits_=None) == E_ARG and f(info_=None) == E_ARG
        for k in ("B_", "L_", "A_", "dh"):
            assert f(**{k: 0}) == E_ARG and f(**{k: -2}) == E_ARG
    assert fwd(ctx_=ptr(ctx) + 4) == E_SHAPE and fwd(ctx_=ptr(ctx) + 2) == E_SHAPE
    assert fwd(dt=F16, ctx2_=ptr(ctx2) + 4) == E_SHAPE
    assert fwd(dt=BF16, ctx2_=ptr(ctx2)) == E_DTYPE and fwd(dt=F32, ctx2_=ptr(ctx2)) == E_DTYPE
    assert bwd(dctx=P + 8) == E_SHAPE and bwd(dqkv_=ptr(dqkv) + 4) == E_SHAPE
    assert bwd(ctx_=None) == E_ARG and bwd(dctx=None) == E_ARG and bwd(lse_=None) == E_ARG
    assert lib.mv_attn_fwd(BF16, P, P, P, None, None, ptr(lse), B, L, A, 64, 0.0, None, None, 0, None, None) == E_ARG
    assert lib.mv_attn_fwd(BF16, P, P, P, ptr(ctx), None, None, B, L, A, 64, 0.0, None, None, 0, None, None) == E_ARG
    assert lib.mv_attn_bwd(BF16, P, P, P, P, P, P, None, ptr(delta), B, L, A, 64, 0.0, None, None, 0, None, None) == E_ARG
    assert lib.mv_attn_bwd(BF16, P, P, P, P, P, P, ptr(dqkv), None, B, L, A, 64, 0.0, None, None, 0, None, None) == E_ARG
    # keep-bit generator
    dm = lambda p=0.1, B_=B, L_=L, A_=A, out=None: lib.mv_attn_dropmask(p, 7, B_, L_, A_, None, ptr(db) if out is None else out, None)
    assert dm(p=0.0) == E_ARG and dm(p=-0.1) == E_ARG and dm(p=1.0) == E_ARG and dm(B_=0) == E_ARG and dm(L_=0) == E_ARG and dm(A_=-1) == E_ARG
    assert lib.mv_attn_dropmask(0.1, 7, B, L, A, None, None, None) == E_ARG
    assert dm(out=ptr(db) + 32) == E_SHAPE and dm(B_=64, L_=4096, A_=16) == E_SHAPE          # 32-bit hash counters / buffer offsets
    # masks
    for nd in (0, 1, 4, -1):
        assert lib.mv_mask_pack(P, nd, B, L, ptr(bits), ptr(info), None) == E_SHAPE
    for bad in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.mv_mask_pack(bad[0], 3, B, L, bad[1], bad[2], None) == E_ARG and lib.mv_mask_build(bad[0], B, L, bad[1], bad[2], None) == E_ARG
    for fn in (lambda b, l: lib.mv_mask_pack(P, 3, b, l, ptr(bits), ptr(info), None), lambda b, l: lib.mv_mask_build(P, b, l, ptr(bits), ptr(info), None)):
        assert fn(0, L) == E_ARG and fn(-1, L) == E_ARG and fn(B, 0) == E_ARG and fn(B, -5) == E_ARG
        assert fn(B, 64 * 64 + 1) == E_SHAPE and fn(1, 1 << 20) == E_SHAPE                    # T = ceil(L / 64) > 64
    for o, b in zip(outs, before):
        assert o.tobytes() == b.tobytes()


def test_rowop_rejects(lib):
    assert lib.mv_layernorm_fwd(BF16, None, F32, P, P, P, None, P, P, 4, 128, 1e-12, None) == E_ARG
    assert lib.mv_layernorm_fwd(BF16, P, F32, P, P, P, None, P, P, 4, 130, 1e-12, None) == E_SHAPE          # H % 4
    emb = lambda **k: lib.mv_embed_fwd(k.get("dt", BF16), P, P, P, k.get("pos", P), P, k.get("img", P), P, P, P, P, P, P, k.get("x2", None), P, P,
                                       P, k.get("B", 2), k.get("N", 4), k.get("T", 8), k.get("H", 128), 1000, k.get("maxpos", 64), 1e-12,
                                       0.0, 0.0, 0, k.get("rowmap", None), k.get("n_rows", 0), None)
    assert emb(B=0) == E_ARG and emb(img=None) == E_ARG and emb(H=130) == E_SHAPE
    assert emb(T=65) == E_SHAPE                                 # text positions 0..T-1 must exist in the position table
    assert emb(rowmap=P, n_rows=0) == E_ARG and emb(rowmap=P, n_rows=2 * 14 + 1) == E_ARG
    assert emb(dt=BF16, x2=P) == E_DTYPE and emb(dt=4) == E_DTYPE
    assert lib.mv_ce_fwd_bwd(None, F32, 8, P, 2, 8, P, None, 0, 0, None, 1.0, None, None) == E_ARG
    assert lib.mv_adamw_step(None, P, P, P, None, None, 16, 1e-3, 0.9, 0.999, 1e-6, 0.0, 1, 1, 1.0, None, None) == E_ARG
    assert lib.mv_gather_rows(BF16, None, 8, P, 2, 8, P, 8, None) == E_ARG
    assert lib.mv_colsum(BF16, None, 8, 2, 8, P, 1, None, None) == E_ARG
    assert lib.mv_cast(None, F32, P, BF16, 16, None) == E_ARG
    assert lib.mv_count_nonfinite(None, 16, P, None) == E_ARG


def test_region_encoder_support_rejects(lib):
    """csrc/mv_conv.hip: one assertion per documented condition of the six entry points (include/medvill.h).  The outputs are real,
    NaN-filled host buffers, compared afterwards: a refused call has written nothing, mv_col_stats' clearing of `stats` included."""
    def nan(n):                              # 64-byte aligned, whatever the allocator returns
        raw = np.empty(n * 4 + 64, dtype=np.uint8)
        a = raw[(-raw.ctypes.data) % 64:][:n * 4].view(np.float32)
        a[...] = np.nan
        return a
    dst, cols, stats, mean, rstd, rmean, rvar, y, pooled = (nan(256) for _ in range(9))
    outs = (dst, cols, stats, mean, rstd, rmean, rvar, y, pooled)
    before = [o.copy() for o in outs]
    ptr = lambda a: a.ctypes.data

    def nhwc(src=P, dst_=None, dt=BF16, B=1, C_=3, H=2, W=2, Cp=8):
        return lib.mv_nchw_to_nhwc(src, ptr(dst) if dst_ is None else dst_, dt, B, C_, H, W, Cp, None)
    assert nhwc(src=None) == E_ARG and lib.mv_nchw_to_nhwc(P, None, BF16, 1, 3, 2, 2, 8, None) == E_ARG
    for k in ("B", "C_", "H", "W"):
        assert nhwc(**{k: 0}) == E_ARG and nhwc(**{k: -1}) == E_ARG, k
    assert nhwc(Cp=2) == E_ARG and nhwc(Cp=0) == E_ARG                     # Cp < C
    assert nhwc(dt=F16) == E_DTYPE and nhwc(dt=3) == E_DTYPE

    def im2col(dt=BF16, src=P, B=1, H=4, W=4, C_=8, kh=3, kw=3, s=1, p=1, dst_=None, ldk=72):
        return lib.mv_im2col(dt, src, B, H, W, C_, kh, kw, s, p, ptr(cols) if dst_ is None else dst_, ldk, None)
    assert im2col(src=None) == E_ARG and lib.mv_im2col(BF16, P, 1, 4, 4, 8, 3, 3, 1, 1, None, 72, None) == E_ARG
    for k in ("B", "H", "W", "C_", "kh", "kw", "s"):
        assert im2col(**{k: 0}) == E_ARG and im2col(**{k: -2}) == E_ARG, k
    assert im2col(p=-1) == E_ARG
    assert im2col(ldk=71) == E_SHAPE and im2col(ldk=64) == E_SHAPE         # ldk < kh*kw*C
    assert im2col(H=2, W=2, kh=7, kw=7, p=1, ldk=392) == E_SHAPE           # an output size that is not positive
    assert im2col(W=1, kw=3, p=0) == E_SHAPE
    assert im2col(dt=F16) == E_DTYPE and im2col(dt=-1) == E_DTYPE

    def col_stats(dt=BF16, x=P, ldx=8, rows=4, C_=8, st=None):
        return lib.mv_col_stats(dt, x, ldx, rows, C_, ptr(stats) if st is None else st, None)
    assert col_stats(x=None) == E_ARG and lib.mv_col_stats(BF16, P, 8, 4, 8, None, None) == E_ARG
    assert col_stats(rows=0) == E_ARG and col_stats(rows=-4) == E_ARG and col_stats(C_=0) == E_ARG and col_stats(ldx=4) == E_ARG
    assert col_stats(C_=6) == E_SHAPE and col_stats(ldx=10) == E_SHAPE     # C % 4, ldx % 4
    assert col_stats(dt=F16) == E_DTYPE and col_stats(dt=5) == E_DTYPE     # and `stats` is not cleared on the way out
    assert col_stats(x=P + 4) == E_SHAPE and col_stats(x=P + 2) == E_SHAPE and col_stats(dt=F32, x=P + 8) == E_SHAPE      # four elements

    def fin(st=P, C_=8, rows=4, mean_=None, rstd_=None, rm=None, rv=None):
        return lib.mv_bn_finalize(st, C_, rows, 1e-5, 0.1, ptr(mean) if mean_ is None else mean_, ptr(rstd) if rstd_ is None else rstd_, rm, rv, None)
    assert fin(st=None) == E_ARG and fin(C_=0) == E_ARG and fin(C_=-8) == E_ARG and fin(rows=0) == E_ARG and fin(rows=-1) == E_ARG
    assert lib.mv_bn_finalize(P, 8, 4, 1e-5, 0.1, None, ptr(rstd), None, None, None) == E_ARG
    assert lib.mv_bn_finalize(P, 8, 4, 1e-5, 0.1, ptr(mean), None, None, None, None) == E_ARG
    assert fin(rm=ptr(rmean)) == E_ARG and fin(rv=ptr(rvar)) == E_ARG      # only one of the two running buffers

    def act(dt=BF16, x=P, xdt=BF16, mean_=P, rstd_=P, gamma=P, beta=P, res=None, y_=None, rows=4, C_=8, use_y=True):
        return lib.mv_bn_act(dt, x, xdt, mean_, rstd_, gamma, beta, res, (ptr(y) if y_ is None else y_) if use_y else None, rows, C_, 1, None)
    for k in ("x", "mean_", "rstd_", "gamma", "beta"):
        assert act(**{k: None}) == E_ARG, k
    assert act(use_y=False) == E_ARG and act(rows=0) == E_ARG and act(rows=-3) == E_ARG and act(C_=0) == E_ARG
    assert act(C_=6) == E_SHAPE                                            # C % 4
    assert act(dt=F32, xdt=BF16) == E_DTYPE                                # f32 out from bf16 in: no such body
    assert act(dt=F16, xdt=F16) == E_DTYPE and act(dt=BF16, xdt=F16) == E_DTYPE and act(dt=F16, xdt=F32) == E_DTYPE and act(dt=4) == E_DTYPE
    assert act(x=P + 4) == E_SHAPE and act(xdt=F32, x=P + 8) == E_SHAPE and act(y_=ptr(y) + 4) == E_SHAPE and act(res=P + 2) == E_SHAPE
    assert act(dt=F32, xdt=F32, y_=ptr(y) + 8) == E_SHAPE and act(dt=F32, xdt=F32, res=P + 8) == E_SHAPE
    for k in ("mean_", "rstd_", "gamma", "beta"):
        assert act(**{k: P + 8}) == E_SHAPE and act(**{k: P + 4}) == E_SHAPE, k

    def pool(dt=BF16, x=P, y_=None, B=1, H=4, W=4, C_=8, use_y=True):
        return lib.mv_maxpool3x3s2(dt, x, (ptr(pooled) if y_ is None else y_) if use_y else None, B, H, W, C_, None)
    assert pool(x=None) == E_ARG and pool(use_y=False) == E_ARG
    for k in ("B", "H", "W", "C_"):
        assert pool(**{k: 0}) == E_ARG and pool(**{k: -1}) == E_ARG, k
    assert pool(C_=6) == E_SHAPE and pool(dt=F16) == E_DTYPE and pool(dt=9) == E_DTYPE
    assert pool(x=P + 4) == E_SHAPE and pool(y_=ptr(pooled) + 4) == E_SHAPE and pool(dt=F32, x=P + 8) == E_SHAPE and pool(dt=F32, y_=ptr(pooled) + 8) == E_SHAPE
    for o, b in zip(outs, before):
        assert o.tobytes() == b.tobytes()


def test_decode_rejects(lib):
    """mv_decode.hip: one assertion per documented condition; every call returns before a launch."""
    gr = lambda **k: lib.mv_gemm_rows(k.get("dt", BF16), k.get("M", 16), k.get("N", 64), k.get("K", 64), k.get("x", P), k.get("ldx", 64), k.get("W", P),
                                      k.get("ldw", 64), k.get("c", P), k.get("ldc", 64), k.get("cdt", F32), k.get("bias", P), k.get("epi", 0),
                                      k.get("r", P), k.get("ldr", 64), k.get("rdt", BF16), None)
    assert gr(x=None) == E_ARG and gr(W=None) == E_ARG and gr(c=None) == E_ARG and gr(M=0) == E_ARG
    assert gr(dt=F32) == E_DTYPE and gr(cdt=3) == E_DTYPE                                   # 16-bit operands only
    assert gr(M=257) == E_SHAPE                                                             # M <= 256
    assert gr(K=48, ldx=48, ldw=48) == E_SHAPE                                              # K % 32
    assert gr(ldx=68) == E_SHAPE and gr(ldw=68) == E_SHAPE                                  # leading dimensions: multiples of 8
    assert gr(ldx=56) == E_SHAPE and gr(ldw=56) == E_SHAPE and gr(ldc=63) == E_SHAPE        # ... and not below K / N
    assert gr(x=P + 8) == E_SHAPE and gr(W=P + 8) == E_SHAPE                                # 16-byte alignment of x and W
    for epi in (4, 5, 6, 7, 8, 10, 11, -1):                                                 # epilogues of mv_gemm this kernel does not have
        assert gr(epi=epi) == E_ARG, epi
    assert gr(epi=1, bias=None) == E_ARG and gr(epi=3, r=None) == E_ARG and gr(epi=3, rdt=5) == E_ARG and gr(epi=3, ldr=63) == E_ARG
    ad = lambda **k: lib.mv_attn_decode(k.get("dt", BF16), k.get("q", P), k.get("ldq", 128), P, P, k.get("ldkv", 128), k.get("slots", P), k.get("lds", 8),
                                        None, k.get("nk", P), k.get("max_nk", 8), P, k.get("ldo", 128), k.get("R", 2), 2, k.get("dh", 64),
                                        k.get("nsplit", 1), k.get("ws", None), k.get("ws_bytes", 0), None)
    assert ad(q=None) == E_ARG and ad(slots=None) == E_ARG and ad(nk=None) == E_ARG and ad(R=0) == E_ARG and ad(max_nk=0) == E_ARG and ad(nsplit=-1) == E_ARG
    assert ad(dt=3) == E_DTYPE
    assert ad(dh=48, ldq=96, ldkv=96, ldo=96) == E_SHAPE                                    # dh must divide 256
    assert ad(dh=256, ldq=512, ldkv=512, ldo=512) == E_SHAPE and ad(dh=2, ldq=4, ldkv=4, ldo=4) == E_SHAPE      # dh <= 128, dh % 4
    assert ad(ldq=127) == E_SHAPE and ad(ldkv=124) == E_SHAPE and ad(ldo=127) == E_SHAPE and ad(lds=0) == E_SHAPE
    assert ad(nsplit=3) == E_WS                                                             # a forced split without a workspace
    assert ad(nsplit=3, ws=P, ws_bytes=(3 * 2 * 2 * 66) * 4 - 4) == E_WS                    # ... or one float short of nsplit * R * A * (dh + 2)
    tk = lambda **k: lib.mv_logprob_topk(k.get("x", P), k.get("ld", 40), k.get("R", 2), k.get("V", 40), k.get("k", 4), -1, k.get("vals", P), k.get("idx", P),
                                         None, None)
    assert tk(x=None) == E_ARG and tk(vals=None) == E_ARG and tk(idx=None) == E_ARG and tk(R=0) == E_ARG and tk(k=0) == E_ARG and tk(ld=39) == E_ARG
    assert tk(k=17) == E_SHAPE                                                              # k <= 16
    assert tk(k=5, V=4) == E_SHAPE                                                          # k <= V
    er = lambda **k: lib.mv_embed_rows(k.get("dt", BF16), k.get("ids", P), P, P, k.get("E", P), P, P, P, P, k.get("out", P), k.get("ldo", 128), k.get("R", 2),
                                       k.get("H", 128), k.get("V", 10), 8, k.get("ntype", 2), 1e-12, None)
    assert er(ids=None) == E_ARG and er(E=None) == E_ARG and er(out=None) == E_ARG and er(R=0) == E_ARG and er(V=0) == E_ARG and er(ntype=0) == E_ARG
    assert er(H=8196, ldo=8196) == E_SHAPE                                                  # H <= 8192
    assert er(ldo=127) == E_SHAPE and er(dt=3) == E_DTYPE


def test_host_mask_check_through_the_raw_abi(lib):
    """Real host work (the only entry point that computes on the CPU): ragged geometry, every family, 1-D masks, threads > samples."""
    out = C.c_longlong(0)
    rng = np.random.default_rng(3)
    for L, n2 in ((37, 7), (64, 18), (95, 4), (512, 38)):
        B = 5
        i, j = np.arange(L).reshape(L, 1), np.arange(L).reshape(1, L)
        vls = rng.integers(n2 + 1, L + 1, size=B)
        for fam in range(5):
            desc = np.stack([np.full(B, fam), np.full(B, n2), vls], 1).astype(np.int32)
            forms = {0: lambda vl: np.broadcast_to(j < vl, (L, L)), 1: lambda vl: (j < n2) | ((i >= n2) & (j >= n2) & (j <= i)),
                     2: lambda vl: (i < n2) | (j < n2) | (j <= i), 3: lambda vl: (i < n2) == (j < n2)}
            if fam == 4:
                m = np.stack([(np.arange(L) < vl) for vl in vls]).astype(np.int64)
            else:
                m = np.stack([forms[fam](vl) for vl in vls]).astype(np.int64)
            m = np.ascontiguousarray(m)
            assert lib.mv_mask_verify_host(m.ctypes.data, m.ndim, desc.ctypes.data, B, L, 8, C.byref(out)) == 0 and out.value == -1, (L, fam)
            idx = tuple(int(rng.integers(0, s)) for s in m.shape)
            m[idx] = 5 if m[idx] == 0 else 0                  # any non-zero value is "visible", like the device packer's `!= 0`
            assert lib.mv_mask_verify_host(m.ctypes.data, m.ndim, desc.ctypes.data, B, L, 3, C.byref(out)) == 0
            assert out.value == int(np.ravel_multi_index(idx, m.shape)), (L, fam, idx)
    m = np.zeros((2, 8, 8), dtype=np.int64)
    d = np.zeros((2, 3), dtype=np.int32)
    assert lib.mv_mask_verify_host(None, 3, d.ctypes.data, 2, 8, 1, C.byref(out)) == E_ARG
    assert lib.mv_mask_verify_host(m.ctypes.data, 4, d.ctypes.data, 2, 8, 1, C.byref(out)) == E_SHAPE
    d[1, 0] = 5
    assert lib.mv_mask_verify_host(m.ctypes.data, 3, d.ctypes.data, 2, 8, 1, C.byref(out)) == E_ARG


def test_comm_rejects(lib):
    """mv_comm_*: argument checks come before RCCL is even loaded (it is bound at run time: the library has no link-time dependency on it)."""
    h = C.c_void_p()
    assert lib.mv_comm_unique_id(None) == E_ARG
    assert lib.mv_comm_init(None, 0, 1, P) == E_ARG and lib.mv_comm_init(C.byref(h), 0, 1, None) == E_ARG
    assert lib.mv_comm_init(C.byref(h), 2, 2, P) == E_ARG and lib.mv_comm_init(C.byref(h), 0, 0, P) == E_ARG
    assert lib.mv_comm_allreduce_async(None, P, 16, F32, None) == E_ARG and lib.mv_comm_wait(None, None) == E_ARG
    assert lib.mv_comm_destroy(None) == E_ARG
    import subprocess
    out = subprocess.run(["bash", "-c", f"readelf -d {_lib.LIB_PATH} | grep NEEDED"], capture_output=True, text=True).stdout
    assert "rccl" not in out and "nccl" not in out, out
