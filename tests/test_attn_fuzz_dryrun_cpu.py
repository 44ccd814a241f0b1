"""Dry run of the bodies of tests/test_attn_fuzz_gpu.py on the CPU: the library's attention entry points are replaced by the torch
stand-in of tests/attn_cases.py (and the mask kernels by the restatement), the device by "cpu".  This checks the harness, not the
kernels: the packing and guard-row bookkeeping, the NaN feeding, the exact expectations and the grading run end to end on every third
case and on the chained cases, so a mistake in the GPU file shows without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import attn_cases as C                        # noqa: E402
import test_attn_fuzz_gpu as T                # noqa: E402

ENC = {torch.float32: C.F32, torch.bfloat16: C.BF16, torch.float16: C.F16}


class StandIn:
    """the entry points the GPU file calls, on CPU tensors"""

    def __init__(self):
        self.planes, self.impl, self.key = 16, 0, 0

    @staticmethod
    def _unpack(bits, B, L):
        W = (L + 31) // 32
        w = bits[:B * L * W].view(B, L, W).to(torch.int64) & 0xFFFFFFFF
        return ((w.unsqueeze(-1) >> torch.arange(32)) & 1).bool().view(B, L, W * 32)[:, :, :L]

    @staticmethod
    def _put(dense, bits, info):
        pb, ti = C.pack_bits(dense).flatten(), C.tile_classes(dense).flatten()
        bits[:pb.numel()] = pb
        info[:ti.numel()] = ti

    def mask_pack(self, arg, bits, info):
        d = arg.bool() if arg.dim() == 3 else arg.bool()[:, None, :].expand(-1, arg.shape[-1], -1)
        self._put(d.contiguous(), bits, info)

    def mask_build(self, desc, B, L, bits, info):
        name = {v: k for k, v in C.FAMILY_ID.items()}
        self._put(torch.stack([C.family_rule(name[int(f)], int(n2), int(vl), L) for f, n2, vl in desc.tolist()]).contiguous(), bits, info)

    def attn_dropmask(self, p, key, B, L, A, out, cu=None):
        self.key = key
        return out

    def attn_keep_mask(self, db, B, L, A):
        g = torch.Generator().manual_seed(self.key & 0xFFFFFFFF)
        return torch.rand((B, A, L, L), generator=g) >= C.drop_thr(0.1, self.planes) / float(1 << self.planes)

    @staticmethod
    def _plan(B, L, cu, qlim):
        Lv = [int(cu[b + 1] - cu[b]) for b in range(B)] if cu is not None else [L] * B
        Lq = [min(v, int(q)) for v, q in zip(Lv, qlim)] if qlim is not None else list(Lv)
        return Lv, Lq, torch.cat([b * L + torch.arange(v) for b, v in enumerate(Lv)])

    @staticmethod
    def _logical(x, B, L, idx):
        out = torch.zeros((B * L, x.shape[-1]), dtype=x.dtype)
        out[idx] = x
        return out.view(B, L, -1)

    def _operand_enc(self, enc, dh):          # the VALU kernels round no operand
        return C.F32 if (dh != C.MFMA_DH or enc == C.F32 or self.impl) else enc

    def attn_fwd(self, qkv, bits, info, ctx, lse, B, L, A, dh, p_drop=0.0, cu=None, total_rows=0, ctx_bf16=None, dropbits=None, qlim=None):
        Lv, Lq, idx = self._plan(B, L, cu, qlim)
        enc, keep, ik = ENC[qkv.dtype], self.attn_keep_mask(None, B, L, A) if p_drop > 0 else None, C.inv_keep(p_drop, self.planes)
        x, dense = self._logical(qkv, B, L, idx), self._unpack(bits, B, L)
        c, ls = C.standin_forward(x, dense, A, Lv, Lq, self._operand_enc(enc, dh), keep, ik, store=enc)
        qrow = torch.arange(L).view(1, L) < torch.tensor(Lq).view(B, 1)
        qs = qrow.reshape(-1)[idx]
        ctx[qs] = c.view(B * L, -1)[idx][qs]
        if ctx_bf16 is not None:
            c2, _ = C.standin_forward(x, dense, A, Lv, Lq, enc, keep, ik, store=C.BF16)
            ctx_bf16[qs] = c2.view(B * L, -1)[idx][qs]
        m = qrow.unsqueeze(1).expand(B, A, L)
        lse.view(B, A, L)[m] = ls[m]

    def attn_bwd(self, qkv, ctx, dctx, lse, bits, info, dqkv, delta, B, L, A, dh, p_drop=0.0, cu=None, total_rows=0, dropbits=None, qlim=None):
        Lv, Lq, idx = self._plan(B, L, cu, qlim)
        enc, keep, ik = ENC[qkv.dtype], self.attn_keep_mask(None, B, L, A) if p_drop > 0 else None, C.inv_keep(p_drop, self.planes)
        lg = lambda t: self._logical(t, B, L, idx)
        dq, dk, dv, dl = C.standin_backward(lg(qkv), lg(ctx), lg(dctx), lse.view(B, A, L), self._unpack(bits, B, L), A, Lv, Lq,
                                            self._operand_enc(enc, dh), keep, ik, store=enc)
        dqkv[:] = torch.cat([dq, dk, dv], -1).view(B * L, -1)[idx]
        m = (torch.arange(L).view(1, L) < torch.tensor(Lq).view(B, 1)).unsqueeze(1).expand(B, A, L)
        delta.view(B, A, L)[m] = dl[m]


@pytest.fixture
def standin(monkeypatch):
    s = StandIn()
    for name in ("mask_pack", "mask_build", "attn_dropmask", "attn_keep_mask", "attn_fwd", "attn_bwd"):
        monkeypatch.setattr(ops, name, getattr(s, name))
    monkeypatch.setattr(ops, "set_attn_planes", lambda p: setattr(s, "planes", p))
    monkeypatch.setattr(ops, "set_attn_order", lambda o: None)
    monkeypatch.setattr(ops, "set_impl", lambda i: setattr(s, "impl", i))
    monkeypatch.setattr(T, "DEV", "cpu")
    monkeypatch.setattr(T, "WORST", {})
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    return s


def test_the_gpu_bodies_run_end_to_end_against_the_stand_in(standin):
    cases = C.all_cases()[::3]
    for c in cases:
        if c["path"] == "mfma":
            T.test_mask_bits_and_tile_classes_equal_the_restatement(c)
        T._forward_and_backward(c)
    for c in (C.mfma_case(13), C.mfma_case(17), C.dense_case(3)):
        T.test_chained_backward_on_the_forward_kernels_own_output(c)
    assert {k[0] for k in T.WORST} == {"ctx", "lse", "delta", "dq", "dk", "dv"} and all(v[0] <= 1.0 for v in T.WORST.values())
    assert any(c.get("lens") for c in cases) and any(c.get("qlim") for c in cases) and any(c["ctx2"] for c in cases) and any(c["order"] for c in cases)
