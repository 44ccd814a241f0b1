"""Cases, dispatch restatement, bound, grading and a torch stand-in of the attention-probability sweep (mv_attn_probs, csrc/mv_attn_probs.hip).

Plain module: nothing here touches the GPU or the HIP library.  It builds on tests/attn_cases.py (generators, masks, inputs, the fp64
forward reference and its p / pd, _score_err, UOP, SAFETY, G_ROWS) without editing it.  tests/test_attn_probs_sweep_gpu.py runs the cases
on the device; tests/test_attn_probs_cases_cpu.py counts the branches, checks the restated constants against the source and validates
the bound with the stand-in, without a GPU.

* dense [B*L] row layout only (every row exists: Lv = L); the kernel is fed the fp64 reference lse rounded to f32, never the forward
  kernel's, so the sweep does not depend on that kernel;
* the reference is ref_forward's p (pd with dropout), the mean over the heads under head_mean;
* the bound, per element, is  SAFETY * (pd * _score_err(s, q, k, |lse|) + store)  -- the f32 arithmetic of one probability against the
  given statistic (its 4 2^-24 (|s| + |lse|) term also covers the rounding of lse to f32) plus the store: f32 2^-24 pd + 2^-126 inv_keep
  (a flushed exponential), 16-bit UOP pd (+ 2^-25 inv_keep for f16 subnormals).  Under head_mean: the mean of the heads' bounds plus
  A 2^-24 mean (A - 1 additions and one division in f32).  Nothing in it is fitted to a kernel's output.
"""
import math
from collections import Counter

import numpy as np
import torch

import attn_cases as C
from attn_cases import BF16, F16, F32, DT, UOP, SAFETY, G_ROWS, U32  # noqa: F401

# ---- constants of mv_attn_probs (tests/test_attn_probs_cases_cpu.py parses the same numbers from the source) ----
MAX_T = 64                    # ceil(L / 64) <= 64
MFMA_DH = 64
VALU_MAX_DH = 128
PATCH_BYTES = 4608            # a wave's 32 x 144-byte LDS patch
VEC_MULTIPLE = {4: 4, 2: 8}   # bytes per output element -> L must be a multiple of this for the 16-byte store route
F32_FLUSH = 2.0 ** -126
NAN = float("nan")

N_FAMILY, N_DENSE, N_VALU = 60, 28, 30
FAMILIES = ("full", "s2s", "bar", "noncross", "1d")


def _finish(cfg, seed):
    """what every case carries: dense rows only, the output encoding and head_mean in turn"""
    cfg.pop("lens", None)
    cfg.pop("qlim", None)
    cfg["ctx2"] = False
    cfg["out"] = F32 if (cfg["enc"] == F32 or (seed // 2) % 2 == 0) else cfg["enc"]
    cfg["hm"] = (seed // 3 + seed) % 2
    cfg["order"] = 0
    return cfg


def family_case(seed):
    """the five mask families at every length of attn_cases.LENGTHS, (B, A) from attn_cases._BA, both 16-bit encodings"""
    rs = np.random.RandomState(72000 + seed)
    L = C.LENGTHS[seed % len(C.LENGTHS)]
    B, A = C._BA[(seed // 3) % len(C._BA)]
    if L >= 321:
        B = min(B, 2)
    fam = FAMILIES[(seed // 15 + seed) % len(FAMILIES)]
    mask = C._family_mask(rs, L, [fam] * B)
    mask["via"] = "pack" if (seed % 3 == 2 or fam == "1d") else "build"
    cfg = dict(seed=seed, path="mfma", enc=(BF16, F16)[(seed // 5 + seed) % 2], B=B, L=L, A=A, dh=MFMA_DH, mask=mask, p=(0.0, 0.1)[(seed // 4) % 2],
               planes=16, vals=C.VALUE_SETS[(seed + seed // 15) % len(C.VALUE_SETS)], dscale=1.0, zero_dctx=False)
    return _finish(cfg, seed)


def dense_case(seed):
    """attn_cases.dense_case (random, holes, split classes, dead rows, ragged all-ones) on padded rows"""
    cfg = C.dense_case(seed)
    cfg["p"] = (0.0, 0.1)[(seed // 2) % 2]
    return _finish(cfg, seed + 1)


def valu_case(seed):
    """the VALU kernel: f32 at impl 0, bf16 / f16 at impl 1, every dh"""
    return _finish(C.valu_case(seed), seed)


def family_cases():
    return [family_case(s) for s in range(N_FAMILY)]


def dense_cases():
    return [dense_case(s) for s in range(N_DENSE)]


def valu_cases():
    return [valu_case(s) for s in range(N_VALU)]


def all_cases():
    return family_cases() + dense_cases() + valu_cases()


def case_id(c):
    return C.case_id(c) + f"-o{c['out']}-hm{c['hm']}"


# =====================================================================================================================
# dispatch restatement (from the dense mask)
# =====================================================================================================================
def out_bytes(cfg):
    return 4 if cfg["out"] == F32 else 2


def dispatch(cfg, dense=None):
    """Counter of the named paths mv_attn_probs takes on this case"""
    c = Counter()
    c["out:f32" if cfg["out"] == F32 else "out:16"] += 1
    c["hm:%d" % cfg["hm"]] += 1
    c["drop" if cfg["p"] > 0 else "nodrop"] += 1
    if cfg["path"] != "mfma":
        c["route:valu:%s" % cfg["enc"]] += 1
        return c
    c["route:mfma:%s" % cfg["enc"]] += 1
    dense = C.dense_mask(cfg) if dense is None else dense
    cls_all = C.tile_classes(dense).numpy()
    B, L = cfg["B"], cfg["L"]
    T = (L + 63) // 64
    c["store:vec" if L % VEC_MULTIPLE[out_bytes(cfg)] == 0 else "store:elem"] += 1
    for b in range(B):
        for tq in range(T):
            for half in range(2):
                q0 = tq * 64 + 32 * half
                if q0 >= L:
                    c["wave_off"] += 1
                    continue
                if q0 + 32 > L:
                    c["ragged_rows"] += 1
                for tk in range(T):
                    c["cls%d" % int(cls_all[b, tq, tk])] += 1
                    if tk * 64 + 64 > L:
                        c["ragged_tail"] += 1
                    c["keypar%d" % (tk & 1)] += 1
    return c


BRANCHES = tuple(["route:mfma:bf16", "route:mfma:f16", "route:valu:f32", "route:valu:bf16", "route:valu:f16", "out:f32", "out:16", "hm:0", "hm:1", "drop",
                  "nodrop", "store:vec", "store:elem", "wave_off", "ragged_rows", "ragged_tail", "cls0", "cls1", "cls2", "keypar0", "keypar1"])


# =====================================================================================================================
# reference and bound
# =====================================================================================================================
def reference(cfg, qkv64, dense, keep):
    """-> dict(ref, bound [B, A, L, L] or [B, L, L] fp64 on qkv64's device, lse32 [B, A, L] f32: what the kernel is fed, r: ref_forward's dict)"""
    A, L, B = cfg["A"], cfg["L"], cfg["B"]
    ik = C.inv_keep(cfg["p"], cfg["planes"])
    r = C.ref_forward(qkv64, dense, A, [L] * B, keep, ik)
    pd = r["pd"]
    e = C._score_err(r["s"], r["q"], r["k"], r["lse"])
    e = torch.where(torch.isfinite(e), e, torch.zeros_like(e))
    if cfg["out"] == F32:
        store = U32 * pd + F32_FLUSH * ik
    else:
        store = UOP[cfg["out"]] * pd + F32_FLUSH * ik + (C.F16_SUBNORMAL_HALF_ULP * ik if cfg["out"] == F16 else 0.0)
    bound = SAFETY * (pd * e + store)
    ref = pd
    if cfg["hm"]:
        ref = pd.mean(dim=1)
        bound = bound.mean(dim=1) + A * U32 * ref
    return dict(ref=ref, bound=bound, lse32=r["lse"].float(), r=r, ik=ik)


def grade(cfg, got, R, guards_ok=True):
    """every assertion of the sweep on one output `got` (the [B, A, L, L] / [B, L, L] tensor the kernel filled): finite everywhere, within
    the bound per element, rows summing to 1 within the summed bound without dropout -> the worst error / bound"""
    assert guards_ok, (cfg, "guard region written")
    assert tuple(got.shape) == tuple(R["ref"].shape), (cfg, tuple(got.shape))
    g = got.double()
    assert bool(torch.isfinite(g).all()), (cfg, "an element inside [L, L] was left unwritten or is not finite")
    ratio, at = C.worst_ratio(g, R["ref"], R["bound"])
    assert ratio <= 1.0, (cfg, "probs", ratio, at)
    if cfg["p"] <= 0:
        dev = (g.sum(-1) - 1.0).abs()
        lim = R["bound"].sum(-1)
        assert bool((dev <= lim).all()), (cfg, "row sums", float((dev / lim).max()))
    return ratio


# =====================================================================================================================
# torch stand-in (CPU only): validates the bound, and with `bug` shows it is not vacuous
# =====================================================================================================================
BUGS = ("mask_word_off_by_one", "tail_off_by_one", "no_inv_keep", "neighbour_lse", "transposed", "hm_wrong_count", "cls0_unwritten")


def standin(cfg, qkv, dense, keep, lse32, bug=None):
    """f32 scores, the exponent in the exp2 form of the MFMA kernel, dropout, the mean over the heads in f32, the store's rounding
    -> the output tensor in the case's encoding (NaN where a planted defect leaves the canary)"""
    B, L, A, dh = cfg["B"], cfg["L"], cfg["A"], cfg["dh"]
    H = A * dh
    ik = C.inv_keep(cfg["p"], cfg["planes"])
    q, k, _ = (C._heads(t.float(), A) for t in qkv.split(H, dim=-1))
    log2e = float(np.float32(1.4426950408889634))
    c2 = float(np.float32(1.0 / math.sqrt(dh)) * np.float32(log2e))
    msk = dense
    if bug == "mask_word_off_by_one":              # the second word of every 64-key tile taken from one word further on (ones past the row)
        msk = dense.clone()
        for k0 in range(0, L, 64):
            n = min(L, k0 + 64) - (k0 + 32)
            if n > 0:
                src = dense[:, :, k0 + 64:k0 + 64 + n]
                msk[:, :, k0 + 32:k0 + 32 + src.shape[-1]] = src
                msk[:, :, k0 + 32 + src.shape[-1]:k0 + 32 + n] = True
    madd = (~msk)[:, None].float() * float(np.float32(C.MASK_ADD) * np.float32(log2e))
    lse = lse32
    if bug == "neighbour_lse":
        lse = torch.roll(lse32, 1, dims=1)
    lse2 = (lse * log2e).unsqueeze(-1)
    p = torch.exp2(((q @ k.transpose(-1, -2)) * c2 + madd) - lse2)
    if keep is not None:
        p = p * keep.float() * (1.0 if bug == "no_inv_keep" else float(np.float32(ik)))
    if bug == "transposed":
        p = p.transpose(-1, -2).contiguous()
    if cfg["hm"]:
        acc = torch.zeros((B, L, L))
        for a in range(A):
            acc = acc + p[:, a]
        p = acc / float(A + (1 if bug == "hm_wrong_count" else 0))
    out = p.to(DT[cfg["out"]])
    if bug == "tail_off_by_one":                   # the last existing key column is never stored: the canary stays
        out[..., L - 1] = NAN
    if bug == "cls0_unwritten":
        cls = C.tile_classes(dense)
        T = (L + 63) // 64
        for b in range(B):
            for tq in range(T):
                for tk in range(T):
                    if int(cls[b, tq, tk]) == 0:
                        out[b, ..., tq * 64:tq * 64 + 64, tk * 64:tk * 64 + 64] = NAN
    return out


def worst(cfg, got, R):
    """error / bound of `got` without asserting (NaN counts as infinite)"""
    return C.worst_ratio(got.double(), R["ref"], R["bound"])[0]
