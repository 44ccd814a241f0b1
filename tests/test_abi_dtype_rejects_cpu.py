"""Which encoding codes every typed entry point refuses, swept over the raw C ABI on the CPU.

Each entry point that picks a kernel instantiation from one or two encoding arguments (MV_F32 = 0, MV_BF16 = 1, MV_F16 = 2) is called
with every combination of {-1, 0, 1, 2, 3} OUTSIDE the set it accepts, with valid small shapes and the fake address P, so that the call
reaches the encoding check and must come back with the exact refusal code.  The accepted sets are literals, restated from the dispatch
chains of csrc/ (they are the `Accept` declarations there); combinations inside a set are never called: that call would launch on P.
The file skips itself where a GPU is present: it tests host code that returns before any launch, and a mistake in a restated set must
not be able to reach a kernel.  mv_colsum is not swept: with accumulate = 0 it enqueues its zero-fill before it looks at the encoding."""
import itertools

import pytest
import torch

import medvill_amd  # noqa: F401
from medvill_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-side refusals only: never run where a call could launch")

E_ARG, E_DTYPE = -1, -3
F32, BF16, F16 = 0, 1, 2
CODES = (-1, 0, 1, 2, 3)
P = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below must return before a launch

ANY = {(F32,), (BF16,), (F16,)}
F32_BF16 = {(F32,), (BF16,)}


def dtype_error(*enc):
    return E_DTYPE


def probs_error(dt, out):          # mv_attn_probs: a bad qkv encoding first, then "out is f32 or qkv's encoding" as an argument error
    return E_DTYPE if dt not in (F32, BF16, F16) else E_ARG


# name -> (call(lib, *encodings), accepted combinations, their number, expected refusal)
CASES = {
    # csrc/mv_rowops.hip
    "mv_layernorm_fwd": (lambda L, d, xd: L.mv_layernorm_fwd(d, P, xd, P, P, P, None, P, P, 4, 128, 1e-12, None),
                         {(F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)}, 5, dtype_error),             # (dtype, x_dtype)
    "mv_layernorm_bwd": (lambda L, d, xd: L.mv_layernorm_bwd(d, P, P, xd, P, P, P, P, P, P, None, 4, 128, None, 0.0, 0, None, None),
                         {(F32, F32), (BF16, F32), (BF16, BF16), (BF16, F16), (F16, F32), (F16, F16)}, 6, dtype_error),
    "mv_embed_fwd": (lambda L, d: L.mv_embed_fwd(d, P, P, P, P, P, P, P, P, P, P, P, P, None, P, P, P, 2, 4, 8, 128, 1000, 64, 1e-12, 0.0, 0.0,
                                                 0, None, 0, None), ANY, 3, dtype_error),
    "mv_embed_bwd": (lambda L, d: L.mv_embed_bwd(d, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 2, 4, 8, 128, 1000, 64, 0, 0.0, 0.0,
                                                 0, None, 0, None, None), ANY, 3, dtype_error),
    "mv_ce_fwd_bwd": (lambda L, ld, dd: L.mv_ce_fwd_bwd(P, ld, 8, P, 2, 8, P, P, dd, 8, None, 1.0, None, None),       # (l_dtype, d_dtype)
                      {(F32, F32), (F32, F16), (F32, BF16), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)}, 7, dtype_error),
    "mv_ce_fwd_bwd[wide rows]": (lambda L, ld, dd: L.mv_ce_fwd_bwd(P, ld, 4096, P, 2, 4096, P, P, dd, 4096, None, 1.0, None, None),
                                 {(F32, F32), (F32, F16), (F32, BF16), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)}, 7, dtype_error),
    "mv_gather_rows": (lambda L, d: L.mv_gather_rows(d, P, 8, P, 2, 8, P, 8, None), ANY, 3, dtype_error),
    "mv_scatter_rows": (lambda L, d: L.mv_scatter_rows(d, P, 8, P, 2, 8, P, 8, 0, None), ANY, 3, dtype_error),
    "mv_add": (lambda L, d: L.mv_add(d, P, P, P, 16, None), ANY, 3, dtype_error),
    "mv_dact": (lambda L, d: L.mv_dact(d, 0, P, P, P, 16, None), ANY, 3, dtype_error),
    "mv_cast2d": (lambda L, s, d: L.mv_cast2d(P, s, 8, P, d, 8, 2, 8, None),                                           # (src, dst): no f16 <-> bf16
                  {(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, F16)}, 7, dtype_error),
    "mv_transpose": (lambda L, d: L.mv_transpose(d, P, 8, P, 8, 8, 8, None), ANY, 3, dtype_error),
    "mv_cast": (lambda L, s, d: L.mv_cast(P, s, P, d, 16, None), set(itertools.product((F32, BF16, F16), repeat=2)), 9, dtype_error),
    # csrc/mv_conv.hip
    "mv_nchw_to_nhwc": (lambda L, d: L.mv_nchw_to_nhwc(P, P, d, 1, 3, 2, 2, 8, None), F32_BF16, 2, dtype_error),
    "mv_im2col": (lambda L, d: L.mv_im2col(d, P, 1, 4, 4, 8, 3, 3, 1, 1, P, 72, None), F32_BF16, 2, dtype_error),
    "mv_col_stats": (lambda L, d: L.mv_col_stats(d, P, 8, 4, 8, P, None), F32_BF16, 2, dtype_error),
    "mv_bn_act": (lambda L, d, xd: L.mv_bn_act(d, P, xd, P, P, P, P, None, P, 4, 8, 1, None),                         # (dtype, x_dtype)
                  {(BF16, BF16), (BF16, F32), (F32, F32)}, 3, dtype_error),
    "mv_maxpool3x3s2": (lambda L, d: L.mv_maxpool3x3s2(d, P, P, 1, 4, 4, 8, None), F32_BF16, 2, dtype_error),
    # csrc/mv_decode.hip
    "mv_gemm_rows": (lambda L, d, cd: L.mv_gemm_rows(d, 16, 64, 64, P, 64, P, 64, P, 64, cd, P, 0, P, 64, BF16, None),  # (dtype, c_dtype)
                     set(itertools.product((BF16, F16), (F32, BF16, F16))), 6, dtype_error),
    "mv_attn_decode": (lambda L, d: L.mv_attn_decode(d, P, 128, P, P, 128, P, 8, None, P, 8, P, 128, 2, 2, 64, 1, None, 0, None),
                       ANY, 3, dtype_error),
    "mv_embed_rows": (lambda L, d: L.mv_embed_rows(d, P, P, P, P, P, P, P, P, P, 128, 2, 128, 10, 8, 2, 1e-12, None), ANY, 3, dtype_error),
    # csrc/mv_vqa.hip, csrc/mv_optim.hip, csrc/mv_lmloss.hip.  The two BCE losses read d_dtype only when dgrad is given (as here)
    "mv_bce_fwd_bwd": (lambda L, d: L.mv_bce_fwd_bwd(P, 8, P, None, 2, 8, None, P, d, 8, None, 1.0, None, None, None, None), ANY, 3, dtype_error),
    "mv_rows_mul": (lambda L, d: L.mv_rows_mul(d, P, 8, P, P, 8, P, 2, 8, P, 8, None), ANY, 3, dtype_error),
    "mv_bce_multilabel": (lambda L, d: L.mv_bce_multilabel(P, 8, P, None, 2, 8, None, P, d, 8, None, 1.0, None, None, None, None),
                          ANY, 3, dtype_error),
    "mv_lm_loss_bwd": (lambda L, d: L.mv_lm_loss_bwd(P, 8, 2, 8, P, P, P, P, 2, 0.0, P, P, P, P, None, P, d, 8, None), ANY, 3, dtype_error),
    # csrc/mv_attn.hip, csrc/mv_attn_probs.hip
    "mv_attn_fwd": (lambda L, d: L.mv_attn_fwd(d, P, P, P, P, None, P, 2, 64, 2, 64, 0.0, None, None, 0, None, None), ANY, 3, dtype_error),
    "mv_attn_bwd": (lambda L, d: L.mv_attn_bwd(d, P, P, P, P, P, P, P, P, 2, 64, 2, 64, 0.0, None, None, 0, None, None), ANY, 3, dtype_error),
    "mv_attn_probs": (lambda L, d, od: L.mv_attn_probs(d, P, P, P, P, P, od, 2, 64, 2, 64, 0.0, None, 0, None),       # (dtype, out_dtype)
                      {(F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)}, 5, probs_error),
}
N_REFUSED = 212         # calls asserted over all cases: sum of 5 ** (encoding arguments) - (accepted combinations)


def _refused(name):
    _, accepted, size, _ = CASES[name]
    assert len(accepted) == size and size > 0, name               # an emptied or shrunken set cannot pass
    n_enc = len(next(iter(accepted)))
    assert all(len(a) == n_enc and all(c in (F32, BF16, F16) for c in a) for a in accepted), name
    return [enc for enc in itertools.product(CODES, repeat=n_enc) if enc not in accepted]


def test_sweep_size():
    assert sum(len(_refused(name)) for name in CASES) == N_REFUSED


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_refused_encodings(lib, name):
    call, _, _, expect = CASES[name]
    for enc in _refused(name):
        assert call(lib, *enc) == expect(*enc), (name, enc)
