"""Sweep of every instantiation and edge of the decode kernels (csrc/mv_decode.hip) against fp64 references (GPU).

The cases, the predicates that name the branches a case takes, the references and the bounds live in tests/decode_cases.py;
tests/test_decode_cases_cpu.py counts the branches.  Every case runs: nothing here may drop one.  Outputs are pre-filled with NaN
(a sentinel for indices), carry padding columns and guard rows before and after, and everything outside the logical extent must
come back untouched.  Input padding holds NaN (or a logit above every real one), so a read past K, N, H or V shows in the result.
All slot and table indices stay inside their allocations.  The assertion messages carry the cfg dict, which reproduces the case.

Bounds (decode_cases.py):
* mv_gemm_rows, f32 output, epilogues without a transcendental: per element 2 K 2^-24 sum_k |x_k w_k| plus one rounding for the bias
  add and one for the residual add (gr_linear_bound); the flat tolerance of tests/test_generate_gpu.py must hold as well;
* GELU epilogue, attention, log-probabilities / lse, embedding: the tolerance the fixed-shape tests assert for the kernel and encoding,
  or 4 x the error plain f32 torch on the CPU makes on the same inputs, whichever is larger (case_tol, ln_case_tol);
* 16-bit outputs: half an ulp of the encoding on top of the f32 bound (out16_bound / store16_bound);
* exact: top-k indices under every tie rule, -10000.0 for a selected penalised column, -inf log-probabilities, zero context rows for
  rows without keys, the constant embedding row, guards and padding.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import decode_cases as C                      # noqa: E402
from rowops_cases import ln_case_tol          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


class Block:
    """A [rows, cols] output inside a flat device allocation: leading dimension ld, `off` elements past a row boundary, guard rows
    before and after, everything pre-filled with `fill`."""

    def __init__(self, rows, cols, ld, dtype, guard_rows, off=0, fill=NAN):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.start = guard_rows * ld + off
        self.flat = torch.full(((rows + 2 * guard_rows) * ld + off + 8,), fill, dtype=dtype, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.before = self.flat.clone()
        self.t = self.flat[self.start:self.start + rows * ld].view(rows, ld)
        inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        inside[self.start:self.start + rows * ld].view(rows, ld)[:, :cols] = True
        self.inside = inside

    def logical(self):
        return self.t[:, :self.cols]

    def outside_untouched(self):
        return torch.equal(_bits(self.flat)[~self.inside], _bits(self.before)[~self.inside])


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / (bound + 1e-300)).max())


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.gr_cases(), ids=lambda c: f"{c['seed']}-M{c['M']}-N{c['N']}-K{c['K']}")
def test_gemm_rows_random_configurations(cfg):
    M, N, K, epi = cfg["M"], cfg["N"], cfg["K"], cfg["epi"]
    info = dict(cfg, branches=C.gr_branches(cfg))
    x_c, W_c, bias_c, res_c = C.gr_inputs(cfg)
    x, W, bias, res = x_c.to(DEV), W_c.to(DEV), bias_c.to(DEV), res_c.to(DEV)
    assert x.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
    out = Block(M, N, cfg["ldc"], C.DT[cfg["cdt"]], C.GR_GUARD_ROWS, off=cfg["c_off"])
    assert out.start == C.gr_c_start(cfg)
    keep = [t.clone() for t in (x, W, res)]
    ops.gemm_rows(x, W, out.t, M=M, N=N, K=K, ldx=cfg["ldx"], ldw=cfg["ldw"], ldc=cfg["ldc"], bias=None if epi == C.EPI_NONE else bias, epi=epi,
                  r=res if epi == C.EPI_BIAS_RES else None, ldr=cfg["ldr"])
    torch.cuda.synchronize()
    assert out.outside_untouched(), info
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(keep, (x, W, res))), info
    got = out.logical()
    assert torch.isfinite(got.float()).all(), info
    x64, W64, b64, r64 = x[:, :K].double(), W[:, :K].double(), bias.double(), res[:, :N].double()
    ref, _, s_abs = C.gr_reference(x64, W64, b64, r64, epi)
    f32_out = cfg["cdt"] == C.F32
    if epi == C.EPI_BIAS_GELU:
        cpu = C.gr_f32_cpu(x_c[:, :K], W_c[:, :K], bias_c, res_c[:, :N], epi).to(DEV)
        bound = torch.full_like(ref, C.case_tol(C.gr_flat_tol(K, True), cpu, ref))
    else:
        bound = C.gr_linear_bound(K, s_abs, b64.expand_as(ref), r64, epi)
    if not f32_out:
        bound = C.store16_bound(ref, cfg["cdt"], bound)
    err = float((got.double() - ref).abs().max())
    worst = _ratio(got, ref, bound)
    print(f"DEV gr {cfg['cdt']} {'gelu' if epi == C.EPI_BIAS_GELU else 'linear'} seed {cfg['seed']} error/bound {worst:.3e} abs {err:.3e}")
    assert worst <= 1.0, (info, worst, err)
    if f32_out or epi != C.EPI_BIAS_RES:                       # the flat tolerance of the fixed-shape test, on every shape
        assert err < C.gr_flat_tol(K, f32_out), (info, err)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.ad_cases(), ids=lambda c: f"{c['seed']}-{c['dt']}-dh{c['dh']}-A{c['A']}-R{c['R']}-{c['mode']}")
def test_attn_decode_random_configurations(cfg):
    R, A, dh, enc = cfg["R"], cfg["A"], cfg["dh"], cfg["dt"]
    H = A * dh
    info = dict(cfg, branches=C.ad_branches(cfg))
    i = C.ad_inputs(cfg)
    plan = i["plan"]
    q = i["q"].to(DEV)
    if cfg["ldkv"] == 2 * H:
        k = i["k"].to(DEV)
        v = k[:, H:]
    else:
        k, v = i["k"].to(DEV), i["v"].to(DEV)
    assert k.stride(0) == cfg["ldkv"] and v.stride(0) == cfg["ldkv"] and q.stride(0) == cfg["ldq"]
    slots, nk = i["slots"].to(DEV), i["nk"].to(DEV)
    slot_row = i["slot_row"].to(DEV) if i["slot_row"] is not None else None
    assert int(slots.min()) >= 0 and int(slots.max()) < k.shape[0] and int(nk.max()) <= slots.shape[1]
    out = Block(R, H, cfg["ldo"], C.DT[enc], C.AD_GUARD_ROWS)
    ws = torch.full((plan["ws_floats"] + 64,), NAN, dtype=torch.float32, device=DEV) if plan["ws_floats"] else None
    ws_before = ws.clone() if ws is not None else None
    ops.attn_decode(q, k, v, slots, nk, out.t, R=R, A=A, dh=dh, max_nk=plan["max_nk"], ldq=cfg["ldq"], ldkv=cfg["ldkv"], ldo=cfg["ldo"],
                    slot_row=slot_row, nsplit=plan["nsplit"], ws=ws[:plan["ws_floats"]] if ws is not None else None)
    torch.cuda.synchronize()
    assert out.outside_untouched(), info
    if ws is not None:
        used = plan["ns"] * R * A * (dh + 2) if plan["ns"] > 1 else 0
        assert torch.equal(_bits(ws[used:]), _bits(ws_before[used:])), info
    got = out.logical()
    assert torch.isfinite(got.float()).all(), info
    ref = C.ad_reference(q, k, v, slots, slot_row, i["nk"], A, dh)
    cpu = C.ad_reference(i["q"], i["k"], i["v"], i["slots"], i["slot_row"], i["nk"], A, dh, dtype=torch.float32).to(DEV)
    empty = (i["nk"] == 0).to(DEV)
    assert bool((got[empty] == 0).all()) and bool((ref[empty] == 0).all()), info
    tol = C.case_tol(C.AD_TOL[enc], cpu, ref)
    err = float((got.double() - ref).abs().max())
    print(f"DEV ad {enc} seed {cfg['seed']} abs {err:.3e} tolerance {tol:.3e}")
    assert err < tol, (info, err, tol)
    if enc != C.F32:                                           # f32 arithmetic, one rounding at the store
        worst = _ratio(got, ref, C.store16_bound(ref, enc, C.case_tol(C.AD_TOL[C.F32], cpu, ref)))
        print(f"DEV ad16 {enc} seed {cfg['seed']} error/bound {worst:.3e}")
        assert worst <= 1.0, (info, worst)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.tk_cases(), ids=lambda c: f"{c['seed']}-V{c['V']}-k{c['k']}-{c['eos_mode']}")
def test_logprob_topk_random_configurations(cfg):
    V, k, ld = cfg["V"], cfg["k"], cfg["ld"]
    info = dict(cfg, branches=C.tk_branches(cfg))
    x_c = C.tk_inputs(cfg)
    R = x_c.shape[0]
    eos = C.tk_eos(cfg)
    x = x_c.to(DEV)
    x_before = x.clone()
    vals = Block(R, k, k, torch.float32, C.TK_GUARD_ROWS)
    idx = Block(R, k, k, torch.int64, C.TK_GUARD_ROWS, fill=C.TK_IDX_SENTINEL)
    lse = Block(1, R, R, torch.float32, C.TK_GUARD_ROWS) if cfg["lse_out"] else None
    ops.logprob_topk(x, k, R=R, V=V, ld=ld, eos_penalty_id=eos, vals=vals.t, idx=idx.t, lse=lse.t if lse else None)
    torch.cuda.synchronize()
    assert vals.outside_untouched() and idx.outside_untouched() and (lse is None or lse.outside_untouched()), info
    assert torch.equal(_bits(x), _bits(x_before)), info
    rv, ri, rl = C.tk_reference(x[:, :V].double(), k, eos)
    got_i, got_v = idx.logical(), vals.logical()
    assert torch.equal(got_i, ri), (info, got_i.tolist(), ri.tolist())
    assert not torch.isnan(got_v).any(), info
    lp_cpu, lse_cpu = C.tk_f32_cpu(x_c[:, :V], k, eos)
    tol = C.case_tol(C.TK_TOL, lp_cpu.to(DEV).gather(1, ri), rv)
    ninf = torch.isinf(rv)
    pen = (ri == eos) if 0 <= eos < V else torch.zeros_like(ninf)
    assert bool((got_v[ninf] == -math.inf).all()), info
    assert bool((got_v[pen] == C.TK_EOS_LOGPROB).all()) and bool((rv[pen] == C.TK_EOS_LOGPROB).all()), info
    rest = ~ninf
    err = float((got_v[rest].double() - rv[rest]).abs().max()) if bool(rest.any()) else 0.0
    print(f"DEV tk values seed {cfg['seed']} abs {err:.3e} tolerance {tol:.3e}")
    assert err <= tol, (info, err, tol)
    if lse is not None:
        ltol = C.case_tol(C.TK_TOL, lse_cpu.to(DEV), rl)
        lerr = float((lse.logical()[0].double() - rl).abs().max())
        print(f"DEV tk lse seed {cfg['seed']} abs {lerr:.3e} tolerance {ltol:.3e}")
        assert lerr <= ltol, (info, lerr, ltol)                # a NaN lse fails here: NaN <= x is false


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.er_cases(), ids=lambda c: f"{c['seed']}-{c['dt']}-H{c['H']}-R{c['R']}")
def test_embed_rows_random_configurations(cfg):
    R, H, enc, eps = cfg["R"], cfg["H"], cfg["dt"], cfg["eps"]
    info = dict(cfg, branches=C.er_branches(cfg))
    i = C.er_inputs(cfg)
    d = {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in i.items()}
    out = Block(R, H, cfg["ldo"], C.DT[enc], C.ER_GUARD_ROWS)
    ops.embed_rows(d["ids"], d["pos"], d["seg"], d["E"], d["P"], d["Ty"], d["gamma"], d["beta"], out.t, R=R, H=H, V=C.ER_V, maxpos=C.ER_MAXPOS,
                   eps=eps, ntype=cfg["ntype"], ldo=cfg["ldo"])
    torch.cuda.synchronize()
    assert out.outside_untouched(), info
    got = out.logical()
    assert torch.isfinite(got.float()).all(), info
    args = ("ids", "pos", "seg", "E", "P", "Ty", "gamma", "beta")
    ref = C.er_reference(*(d[n] for n in args), eps)
    cpu = C.er_reference(*(i[n] for n in args), eps, dtype=torch.float32).to(DEV)
    only_const = R == 1 and i["const"] is not None             # nothing but the constant row: it is compared exactly below
    tol = C.ER_TOL if only_const else ln_case_tol(C.ER_TOL, cpu, ref, i["const"])
    if enc == C.F32:
        err = C.rowrel(got, ref)
        print(f"DEV er f32 seed {cfg['seed']} row-relative {err:.3e} tolerance {tol:.3e}")
        assert err < tol, (info, err, tol)
    else:
        worst = _ratio(got, ref, C.out16_bound(ref, enc, tol))
        print(f"DEV er16 {enc} seed {cfg['seed']} error/bound {worst:.3e}")
        assert worst <= 1.0, (info, worst)
    if i["const"] is not None:                                 # the constant row: mean exact, variance 0, y is beta rounded once
        assert torch.equal(_bits(got[i["const"]]), _bits(d["beta"].to(C.DT[enc]))), info
