"""Sweep of every branch of mv_attn_probs (csrc/mv_attn_probs.hip) against the fp64 reference (GPU).

Cases, restated dispatch, reference, bound and grading live in tests/attn_probs_cases.py; tests/test_attn_probs_cases_cpu.py counts the
branches and validates the bound without a GPU.  Every case runs.  The output sits inside one allocation, pre-filled with NaN, with
guard regions before and after that must come back untouched; every element inside [L, L] must be written (the NaN canary is gone) and
lie within the per-element bound; without dropout every row sums to 1 within the summed bound.  The kernel is fed the fp64 reference's
lse rounded to f32 and, with dropout, the keep-bits of mv_attn_dropmask (decoded by hip_ops.attn_keep_mask for the reference).
The MFMA kernel is also run against the plain VALU kernel through the debug library's impl knob.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import attn_cases as C                        # noqa: E402
import attn_probs_cases as P                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                                   # guard elements before and after the output
WORST = {}


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _make_mask(cfg):
    B, L = cfg["B"], cfg["L"]
    W, T = (L + 31) // 32, (L + 63) // 64
    how, arg = C.mask_argument(cfg)
    bits = torch.zeros((B * L * W,), dtype=torch.int32, device=DEV)
    info = torch.zeros((B * T * T,), dtype=torch.uint8, device=DEV)
    if how == "build":
        ops.mask_build(arg.to(DEV), B, L, bits, info)
    else:
        ops.mask_pack(arg.to(DEV), bits, info)
    return bits, info


def _setup(cfg):
    B, L, A = cfg["B"], cfg["L"], cfg["A"]
    qkv_c, _ = C.inputs(cfg)
    s = dict(qkv=qkv_c.to(DEV).view(B * L, -1).contiguous(), dense=C.dense_mask(cfg).to(DEV), db=None, keep=None)
    s["bits"], s["info"] = _make_mask(cfg)
    if cfg["p"] > 0:
        s["db"] = torch.zeros(ops.dropbits_numel(B, L, A) + 16, dtype=torch.int32, device=DEV)
        ops.attn_dropmask(cfg["p"], 0xA77E + cfg["seed"], B, L, A, s["db"])
        s["keep"] = ops.attn_keep_mask(s["db"], B, L, A)
    s["R"] = P.reference(cfg, qkv_c.to(DEV).double(), s["dense"], s["keep"])
    return s


def _run(cfg, s, impl):
    """-> (the output view, guards untouched?)"""
    B, L, A, dh = cfg["B"], cfg["L"], cfg["A"], cfg["dh"]
    n = B * (1 if cfg["hm"] else A) * L * L
    flat = torch.full((n + 2 * GUARD,), P.NAN, dtype=C.DT[cfg["out"]], device=DEV)
    before = flat.clone()
    out = flat[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    try:
        ops.set_impl(impl)
        ops.attn_probs(s["qkv"], s["bits"], s["info"], s["R"]["lse32"].contiguous(), out, B, L, A, dh, p_drop=cfg["p"], dropbits=s["db"],
                       head_mean=bool(cfg["hm"]))
        torch.cuda.synchronize()
    finally:
        ops.set_impl(0)
    ok = torch.equal(_bits(flat[:GUARD]), _bits(before[:GUARD])) and torch.equal(_bits(flat[GUARD + n:]), _bits(before[GUARD + n:]))
    return out.view((B, L, L) if cfg["hm"] else (B, A, L, L)), ok


def _sweep(cfg):
    s = _setup(cfg)
    impl = 1 if (cfg["path"] == "valu" and cfg["enc"] != C.F32) else 0
    got, ok = _run(cfg, s, impl)
    ratio = P.grade(cfg, got, s["R"], guards_ok=ok)
    key = (cfg["path"], cfg["enc"], cfg["out"], cfg["hm"])
    if ratio > WORST.get(key, (-1.0, None))[0]:
        WORST[key] = (ratio, P.case_id(cfg))
    print(f"DEV attn_probs error/bound {ratio:.3e}  {P.case_id(cfg)}")
    return s, got


@pytest.mark.parametrize("cfg", P.family_cases(), ids=P.case_id)
def test_family_masks_every_length_encoding_and_option(cfg):
    _sweep(cfg)


@pytest.mark.parametrize("cfg", P.dense_cases(), ids=P.case_id)
def test_dense_masks_holes_split_classes_dead_rows_ragged_ones(cfg):
    _sweep(cfg)


@pytest.mark.parametrize("cfg", P.valu_cases(), ids=P.case_id)
def test_valu_kernel_every_dh_and_encoding(cfg):
    _sweep(cfg)


@pytest.mark.parametrize("cfg", [P.family_case(s) for s in (3, 10, 25, 44)] + [P.dense_case(s) for s in (2, 5, 12, 17)], ids=P.case_id)
def test_mfma_kernel_against_the_simple_kernel(cfg):
    """the same call through the debug library's impl knob: both within the bound of the reference, hence within twice the bound of each other"""
    s, got = _sweep(cfg)
    simple, ok = _run(cfg, s, 1)
    P.grade(cfg, simple, s["R"], guards_ok=ok)
    diff = (got.double() - simple.double()).abs()
    assert bool((diff <= 2.0 * s["R"]["bound"]).all()), (cfg, float((diff / s["R"]["bound"]).nan_to_num(0.0).max()))


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for key in sorted(WORST):
        print(f"WORST attn_probs {key} {WORST[key][0]:.3f}   {WORST[key][1]}")
