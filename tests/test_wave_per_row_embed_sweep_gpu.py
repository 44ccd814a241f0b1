"""Sweep of embed_fwd_kernel / embed_bwd_kernel (csrc/mv_rowops.hip, behind mv_embed_fwd / mv_embed_bwd) against fp64 references (GPU).

The cases, the restatement of what a case takes through the launchers and emb_decode, the references, the bounds and the checks
themselves live in tests/embed_cases.py; tests/test_embed_cases_cpu.py counts the branches and runs the same checks on a plain f32
torch implementation.  Every case runs: nothing here may drop one.  Every output sits in a NaN-filled buffer between guard elements,
every input is compared bit for bit before and after, and the assertion messages carry the cfg dict, which reproduces the case.

Forward: pre bit-exact against (e.float() + p.float()) + t.float(); mean / rstd as the LayerNorm forward sweep bounds them; x0 per row
(f32: 1e-5 or 4 x plain f32 torch on the CPU, 16-bit: half an ulp on top), dropped elements exactly zero, nothing past n_rows written.
Backward: fed with pre from the f32 expression and the fp64 reference's mean / rstd rounded to f32, so a forward bug can neither mask nor
cause a failure; the five f32 accumulators start from a random previous gradient and are checked per element against a bound that
holds for any order of the atomic adds (embed_cases.emb_bwd_bounds); rows nothing maps to, and the pad row, stay bit-unchanged; dimg is
written for the packed image rows only.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import embed_cases as C                       # noqa: E402
from test_rowops_fuzz_gpu import Guarded      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {C.F32: 0, C.BF16: 1, C.F16: 2}        # MV_F32 / MV_BF16 / MV_F16
IDS = ("cls", "sep", "txt", "seg", "img_pos", "rowmap")
TABLES = ("E", "P", "Ty", "imgproj", "gamma", "beta")


def _device_inputs(inp):
    d = {k: (None if inp[k] is None else inp[k].to(DEV)) for k in IDS + TABLES + ("dx0",)}
    return d, {k: (None if v is None else v.clone()) for k, v in d.items()}


def _unchanged(d, before):
    return all(v is None or C.same_bits(v, before[k]) if v is None or v.is_floating_point() else torch.equal(v, before[k]) for k, v in d.items())


def _forward(cfg, d, n_rows, p_drop, p_drop_img):
    B, N, T, H, V, maxpos = cfg["B"], cfg["N"], cfg["T"], cfg["H"], cfg["V"], cfg["maxpos"]
    rows = B * C.emb_L(cfg)
    buf = dict(x0=Guarded(rows * H, C.DT[cfg["dt"]]), x0_bf16=Guarded(rows * H, torch.bfloat16) if cfg["x0_bf16"] else None,
               pre=Guarded(rows * H, torch.float32), mean=Guarded(rows, torch.float32), rstd=Guarded(rows, torch.float32))
    ops.embed_fwd(CODE[cfg["dt"]], d["cls"], d["txt"], d["seg"], d["img_pos"], d["sep"], d["imgproj"], d["E"], d["P"], d["Ty"], d["gamma"],
                  d["beta"], buf["x0"].t, buf["pre"].t, buf["mean"].t, buf["rstd"].t, B, N, T, H, V, maxpos, cfg["eps"], p_drop=p_drop,
                  drop_key=cfg["drop_key"], rowmap=d["rowmap"], n_rows=n_rows if d["rowmap"] is not None else 0,
                  x0_bf16=buf["x0_bf16"].t if buf["x0_bf16"] else None, p_drop_img=p_drop_img)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("cfg", C.emb_cases(), ids=lambda c: f"{c['seed']}-{c['dt']}-H{c['H']}-B{c['B']}N{c['N']}T{c['T']}-{c['rowmap']}")
def test_embedding_random_configurations(cfg):
    B, N, T, H, V, maxpos = cfg["B"], cfg["N"], cfg["T"], cfg["H"], cfg["V"], cfg["maxpos"]
    info = dict(cfg, branches=C.emb_branches(cfg))
    inp = C.emb_inputs(cfg)
    n = inp["n_rows"]
    ref = C.emb_reference(cfg, inp, DEV)
    fwd_tol, bwd_tol = C.emb_tolerances(cfg, inp, ref)
    d, before = _device_inputs(inp)
    # ---- forward
    buf = _forward(cfg, d, n, cfg["p_drop"], cfg["p_drop_img"])
    assert all(b is None or b.guards_untouched() for b in buf.values()), info
    assert _unchanged(d, before), info
    C.check_forward(cfg, inp, ref, {k: (None if b is None else b.t) for k, b in buf.items()}, fwd_tol)
    if cfg["p_drop"] > 0 or cfg["p_drop_img"] > 0:            # pre, mean and rstd do not depend on the dropout
        clean = _forward(cfg, d, n, 0.0, 0.0)
        for k in ("pre", "mean", "rstd"):
            per = H if k == "pre" else 1
            assert C.same_bits(clean[k].t[:n * per], buf[k].t[:n * per]), (info, k, "changes with the dropout")
    # ---- backward, on inputs of its own: pre from the f32 expression, mean / rstd of the fp64 reference rounded to f32
    pre_in, mean_in, rstd_in = ref["pre_f32"].contiguous(), ref["mean"].float().contiguous(), ref["rstd"].float().contiguous()
    stats_before = (pre_in.clone(), mean_in.clone(), rstd_in.clone())
    acc = {}
    for k in C.ACC:
        acc[k] = Guarded(inp["prev"][k].numel(), torch.float32)
        acc[k].t.copy_(inp["prev"][k].to(DEV).reshape(-1))
    dimg = Guarded(B * N * H, C.DT[cfg["dt"]]) if N else None
    us = None if cfg["unscale"] is None else torch.tensor([cfg["unscale"]], dtype=torch.float32, device=DEV)
    ops.embed_bwd(CODE[cfg["dt"]], d["dx0"], pre_in, mean_in, rstd_in, d["gamma"], d["cls"], d["txt"], d["seg"], d["img_pos"], d["sep"],
                  acc["dE"].t, acc["dP"].t, acc["dTy"].t, acc["dg"].t, acc["db"].t, dimg.t if dimg else None, B, N, T, H, V, maxpos,
                  pad_token_id=cfg["pad"], p_drop=cfg["p_drop"], drop_key=cfg["drop_key"], rowmap=d["rowmap"],
                  n_rows=n if d["rowmap"] is not None else 0, unscale=us, p_drop_img=cfg["p_drop_img"])
    torch.cuda.synchronize()
    assert all(b.guards_untouched() for b in acc.values()) and (dimg is None or dimg.guards_untouched()), info
    assert _unchanged(d, before), info
    assert all(C.same_bits(a, b) for a, b in zip((pre_in, mean_in, rstd_in), stats_before)), info
    out = {k: acc[k].t.view(inp["prev"][k].shape) for k in C.ACC}
    out["dimg"] = dimg.t if dimg else None
    C.check_backward(cfg, inp, ref, out, bwd_tol)


def test_embedding_rejects():
    """arguments the launchers refuse before any launch (device pointers real): the outputs stay as they were"""
    cfg = dict(C.emb_case(5), H=132, dt=C.BF16, x0_bf16=False, B=2, N=1, T=3, img_pos=True, rowmap="none", V=50, maxpos=8, bad=False)
    inp = C.emb_inputs(cfg)
    d, _ = _device_inputs(inp)
    B, N, T, H, V, maxpos = 2, 1, 3, 132, 50, 8
    rows = B * C.emb_L(cfg)
    nan = lambda n, dt: torch.full((n,), float("nan"), dtype=dt, device=DEV)      # noqa: E731
    x0, x0b, pre, mean, rstd = nan(rows * 2052, torch.bfloat16), nan(rows * 2052, torch.bfloat16), nan(rows * 2052, torch.float32), \
        nan(rows, torch.float32), nan(rows, torch.float32)
    rowmap = torch.arange(rows, dtype=torch.int32, device=DEV)

    def fwd(H=H, T=T, maxpos=maxpos, rowmap=None, n_rows=0, x0_bf16=None, tables=d):
        ops.embed_fwd(1, d["cls"], d["txt"], d["seg"], d["img_pos"], d["sep"], tables["imgproj"], tables["E"], tables["P"], tables["Ty"],
                      tables["gamma"], tables["beta"], x0, pre, mean, rstd, B, N, T, H, V, maxpos, 1e-12, rowmap=rowmap, n_rows=n_rows,
                      x0_bf16=x0_bf16)
    acc = {k: v.to(DEV).clone() for k, v in inp["prev"].items()}
    dimg = nan(B * N * 2052, torch.bfloat16)

    def bwd(H=H, rowmap=None, n_rows=0):
        ops.embed_bwd(1, d["dx0"], pre, mean, rstd, d["gamma"], d["cls"], d["txt"], d["seg"], d["img_pos"], d["sep"], acc["dE"], acc["dP"],
                      acc["dTy"], acc["dg"], acc["db"], dimg, B, N, T, H, V, maxpos, rowmap=rowmap, n_rows=n_rows)
    with pytest.raises(RuntimeError, match="MV_E_DTYPE"):
        fwd(x0_bf16=x0b)                                        # the bf16 shadow is f16's alone
    with pytest.raises(RuntimeError, match="MV_E_SHAPE"):
        fwd(T=maxpos + 1)                                       # text positions 0..T-1 must exist
    for n_rows in (0, rows + 1):
        with pytest.raises(RuntimeError, match="MV_E_ARG"):
            fwd(rowmap=rowmap, n_rows=n_rows)
        with pytest.raises(RuntimeError, match="MV_E_ARG"):
            bwd(rowmap=rowmap, n_rows=n_rows)
    with pytest.raises(RuntimeError, match="MV_E_SHAPE"):
        fwd(H=2052)
    with pytest.raises(RuntimeError, match="MV_E_SHAPE"):
        bwd(H=2052)
    torch.cuda.synchronize()
    for t in (x0, x0b, pre, mean, rstd, dimg):
        assert bool(torch.isnan(t.float()).all())
    assert all(C.same_bits(acc[k], inp["prev"][k].to(DEV)) for k in acc)
