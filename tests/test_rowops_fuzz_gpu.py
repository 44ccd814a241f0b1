"""Sweep of every dispatch branch of the row kernels (csrc/mv_rowops.hip) against fp64 references (GPU).

The cases, the predicates that say which launcher branch a case takes and the references live in tests/rowops_cases.py;
tests/test_rowops_cases_cpu.py counts the branches.  Every case runs: nothing here may drop one.  Outputs are pre-filled with
NaN, leading dimensions carry padding, and everything outside the logical extent must come back untouched (except where the ABI
says zero-filled).  The assertion messages carry the cfg dict, which reproduces the case.

Tolerances (rowops_cases.py: sum_bound, out16_bound, aw_bounds):
* data movement and single-rounding element-wise results: bit-exact against the torch expression with the same f32 operation;
* f32 reductions: 2 n 2^-24 sum|terms| per output element, sum|terms| from the fp64 reference;
* 16-bit outputs of f32 math: half an ulp of the encoding on top of the kernel's f32 tolerance;
* f32 LayerNorm and cross-entropy outputs: the tolerances tests/test_kernels_gpu.py asserts for the same kernels (1e-5 forward and
  cross-entropy gradient, 1e-4 backward, 1e-3 on the loss sum), applied per row so that one wrong row cannot hide behind the others.
  A LayerNorm case takes the larger of that and 4 x the error plain f32 torch on the CPU makes on the same inputs
  (rowops_cases.ln_case_tol); the column sums of its backward add the f32 error of their terms, derived from the arithmetic
  (rowops_cases.ln_term_errors), to the summation bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import rowops_cases as C                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 16
CE_PAD_LOGIT = 3.0e4        # what the columns V..ld-1 of the logits hold: read as a logit it would be every row's maximum

LN_FWD_TOL, LN_BWD_TOL, CE_GRAD_TOL, CE_NLL_TOL, DACT_TOL = 1e-5, 1e-4, 1e-5, 1e-3, 1e-5      # tests/test_kernels_gpu.py


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_values(got, exp):
    """bit-for-bit, except that a NaN only has to be a NaN"""
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    return bool(((_bits(got) == _bits(exp)) | (torch.isnan(got) & torch.isnan(exp))).all())


class Guarded:
    """A flat device buffer of n elements starting `off` elements into its allocation, with guard elements on both sides;
    everything is pre-filled with NaN (or `fill`)."""

    def __init__(self, n, dtype, off=0, fill=NAN):
        self.off, self.n = off, n
        self.flat = torch.full((off + n + GUARD,), fill, dtype=dtype, device=DEV)
        self.before = self.flat.clone()
        self.t = self.flat[off:off + n]

    def guards_untouched(self):
        return torch.equal(_bits(self.flat[:self.off]), _bits(self.before[:self.off])) and \
            torch.equal(_bits(self.flat[self.off + self.n:]), _bits(self.before[self.off + self.n:]))


_rowrel = C.rowrel


def _within(got, ref, bound):
    """-> (ok, worst ratio error / bound)"""
    r = ((got.double() - ref).abs() / (bound + 1e-300)).max()
    return bool(r <= 1.0), float(r)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.ce_cases(), ids=lambda c: f"{c['seed']}-V{c['V']}-R{c['R']}")
def test_cross_entropy_random_configurations(cfg):
    V, R, ld, ldd = cfg["V"], cfg["R"], cfg["ld"], cfg["ldd"]
    branch, why = C.ce_branch(cfg)
    x, lab, _ = C.ce_inputs(cfg)
    ldt = C.DT[cfg["ldt"]]
    lbuf = Guarded(R * ld, ldt, cfg["l_off"], fill=CE_PAD_LOGIT)
    logits = lbuf.t.view(R, ld)
    logits[:, :V] = x.to(DEV)
    lbefore = lbuf.flat.clone()
    labels = lab.to(torch.int32).to(DEV)
    out = torch.zeros(3, dtype=torch.float32, device=DEV)
    dbuf = Guarded(R * ldd, C.DT[cfg["ddt"]], cfg["d_off"]) if cfg["ddt"] else None
    gs_dev, gs_host, ls_dev, scale = C.ce_scales(cfg)
    gs_t = torch.tensor([gs_dev], dtype=torch.float32, device=DEV) if gs_dev is not None else None
    ls_t = torch.tensor([ls_dev], dtype=torch.float32, device=DEV) if ls_dev is not None else None
    ops.ce_fwd_bwd(logits, ld, labels, R, V, out, dbuf.t if dbuf else None, ldd, grad_scale_dev=gs_t, grad_scale=gs_host, loss_scale_dev=ls_t)
    nll, cnt, hits, grad = C.ce_reference(logits[:, :V].double(), lab.to(DEV), scale)
    info = dict(cfg, branch=branch, why=why)
    got = out.tolist()
    print(f"ce {cfg['seed']} {branch}: nll {got[0]:.6f} ref {nll:.6f} count {got[1]} ref {cnt} hits {got[2]} ref {hits}")
    assert torch.equal(lbuf.flat, lbefore), info                                           # the logits are read-only
    assert got[1] == float(cnt) and got[2] == float(hits), (info, got, cnt, hits)
    assert abs(got[0] - nll) < CE_NLL_TOL * max(1.0, abs(nll)), (info, got[0], nll)
    if cnt == 0:
        assert got[0] == 0.0, info
    if dbuf is None:
        return
    dl = dbuf.t.view(R, ldd)
    assert dbuf.guards_untouched(), info
    assert torch.isfinite(dl.float()).all(), info
    assert bool((dl[:, V:] == 0).all()), info                                              # zero-filled by the ABI
    valid = ((lab >= 0) & (lab < V)).to(DEV)
    assert bool((dl[~valid] == 0).all()), info                                             # ignored and out-of-range labels: a zero row
    if cfg["ddt"] == C.F32:
        err = _rowrel(dl[:, :V], grad)
        print(f"    f32 gradient row-relative error {err:.3e}")
        assert err < CE_GRAD_TOL, (info, err)
    else:
        ok, worst = _within(dl[:, :V], grad, C.out16_bound(grad, cfg["ddt"], CE_GRAD_TOL))
        print(f"    {cfg['ddt']} gradient error / bound {worst:.3f}")
        assert ok, (info, worst)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.ln_cases(), ids=lambda c: f"{c['seed']}-M{c['M']}-H{c['H']}-v{c['variant']}")
def test_layernorm_random_configurations(cfg):
    M, H, eps = cfg["M"], cfg["H"], cfg["eps"]
    info = dict(cfg, fwd=C.ln_fwd_branches(cfg), bwd=C.ln_bwd_branches(cfg))
    x_c, gamma_c, beta_c, dy_c, const = C.ln_inputs(cfg)
    x, gamma, beta, dy = x_c.to(DEV), gamma_c.to(DEV), beta_c.to(DEV), dy_c.to(DEV)
    ref = C.ln_reference(x.double(), gamma.double(), beta.double(), dy.double(), eps)
    # the f32 tolerances of this case: those of tests/test_kernels_gpu.py, or 4 x what plain f32 torch on the CPU misses on these inputs
    y_cpu, dx_cpu = C.ln_f32_cpu(x_c, gamma_c, beta_c, dy_c, eps)
    fwd_tol = C.ln_case_tol(LN_FWD_TOL, y_cpu.to(DEV), ref["y"], const)
    bwd_tol = C.ln_case_tol(LN_BWD_TOL, dx_cpu.to(DEV), ref["dx"], const)
    print(f"ln {cfg['seed']} tolerances: forward {fwd_tol:.3e} backward {bwd_tol:.3e}")
    # ---- forward
    ybuf = Guarded(M * H, C.DT[cfg["ydt"]])
    y2buf = Guarded(M * H, torch.bfloat16) if cfg["y_bf16"] else None
    mean, rstd = Guarded(M, torch.float32), Guarded(M, torch.float32)
    ops.layernorm_fwd(x, gamma, beta, ybuf.t, mean.t, rstd.t, M, H, eps, y_bf16=y2buf.t if y2buf else None)
    for b in (ybuf, mean, rstd) + ((y2buf,) if y2buf else ()):
        assert b.guards_untouched(), info
    y = ybuf.t.view(M, H)
    assert torch.isfinite(y.float()).all() and torch.isfinite(mean.t).all() and torch.isfinite(rstd.t).all(), info
    if cfg["ydt"] == C.F32:
        err = _rowrel(y, ref["y"])
        print(f"ln {cfg['seed']} fwd f32 row-relative error {err:.3e}")
        assert err < fwd_tol, (info, err, fwd_tol)
    else:
        ok, worst = _within(y, ref["y"], C.out16_bound(ref["y"], cfg["ydt"], fwd_tol))
        print(f"ln {cfg['seed']} fwd {cfg['ydt']} error / bound {worst:.3f}")
        assert ok, (info, worst)
    if y2buf:
        ok, worst = _within(y2buf.t.view(M, H), ref["y"], C.out16_bound(ref["y"], C.BF16, fwd_tol))
        assert ok, (info, "y_bf16", worst)
    xmax = x.double().abs().amax(dim=1)
    assert bool(((mean.t.double() - ref["mean"]).abs() <= LN_FWD_TOL * xmax).all()), info
    assert bool(((rstd.t.double() - ref["rstd"]).abs() <= LN_BWD_TOL * ref["rstd"]).all()), info
    if const is not None:                                       # the constant row: y is beta, rounded once
        assert _same_bits(y[const], beta.to(C.DT[cfg["ydt"]])), info
    # ---- backward, fed with the reference's own statistics (f32), so that it is judged on its own
    mean_r, rstd_r = ref["mean"].float(), ref["rstd"].float()
    us = cfg["unscale"]
    us_t = torch.tensor([us], dtype=torch.float32, device=DEV) if us != 1.0 else None
    ddt = C.DT[cfg["ddt"]]
    dxbuf = Guarded(M * H, ddt)
    ddbuf = Guarded(M * H, ddt) if cfg["p_drop"] > 0 else None
    start = {k: torch.randn((H,), generator=torch.Generator().manual_seed(cfg["seed"] + i)).to(DEV) for i, k in enumerate(("dg", "db", "cs"))}
    acc = {k: Guarded(H, torch.float32) for k in start}
    for k in acc:
        acc[k].t.copy_(start[k])
    try:
        ops.set_rowops_variant(cfg["variant"])
        ops.layernorm_bwd(dy, x, mean_r, rstd_r, gamma, dxbuf.t, acc["dg"].t, acc["db"].t, acc["cs"].t, M, H,
                          dx_drop=ddbuf.t if ddbuf else None, p_drop=cfg["p_drop"], drop_key=cfg["drop_key"], unscale=us_t)
        torch.cuda.synchronize()
    finally:
        ops.set_rowops_variant(0)
    for b in (dxbuf,) + tuple(acc.values()) + ((ddbuf,) if ddbuf else ()):
        assert b.guards_untouched(), info
    dx = dxbuf.t.view(M, H)
    assert torch.isfinite(dx.float()).all(), info
    dx_ref = ref["dx"]
    if cfg["p_drop"] > 0:
        keep, sc = ops.dropout_mask(cfg["p_drop"], cfg["drop_key"], M * H, DEV)
        keep = keep.view(M, H).bool()
        assert np.array_equal(keep.cpu().numpy().ravel(), C.dm_restated(cfg["p_drop"], cfg["drop_key"], M * H).astype(bool)), info
        dd_ref = dx_ref * keep * sc
    else:
        dd_ref = dx_ref
    outs = [("dx", dx, dx_ref)] + ([("dx_drop", ddbuf.t.view(M, H), dd_ref)] if ddbuf else [])
    for name, got, want in outs:
        if cfg["ddt"] == C.F32:
            err = _rowrel(got, want)
            print(f"    bwd {name} f32 row-relative error {err:.3e}")
            assert err < bwd_tol, (info, name, err, bwd_tol)
        else:
            ok, worst = _within(got, want, C.out16_bound(want, cfg["ddt"], bwd_tol))
            print(f"    bwd {name} {cfg['ddt']} error / bound {worst:.3f}")
            assert ok, (info, name, worst)
    if ddbuf:
        assert bool((ddbuf.t.view(M, H)[~keep] == 0).all()), info                       # the keep pattern itself
    # column accumulators: out = start + unscale * sum over rows: the summation bound over M rows plus the start value, plus the f32
    # error of the terms themselves, derived from their arithmetic (rowops_cases.ln_term_errors; none for dbeta)
    dy64 = dy.double()
    terms = {"dg": dy64 * ref["xhat"], "db": dy64, "cs": dd_ref}
    term_err = C.ln_term_errors(x.double(), dy64, ref, dd_ref, const)
    for k in ("dg", "db", "cs"):
        want = start[k].double() + us * terms[k].sum(0)
        mag = start[k].double().abs() + us * terms[k].abs().sum(0)
        ok, worst = _within(acc[k].t, want, C.sum_bound(M + 2, mag) + us * term_err[k].sum(0))
        print(f"    bwd {k} error / bound {worst:.3f}")
        assert ok, (info, k, worst)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.gs_cases(), ids=lambda c: f"{c['seed']}-{c['op']}-{c['dt']}-H{c['H']}-R{c['R']}")
def test_gather_scatter_random_configurations(cfg):
    H, R, lds, ldd, dt = cfg["H"], cfg["R"], cfg["lds"], cfg["ldd"], C.DT[cfg["dt"]]
    info = dict(cfg, branches=C.gs_branches(cfg))
    g = torch.Generator().manual_seed(cfg["seed"])
    rows = C.gs_rows(cfg).to(DEV)
    rows32 = rows.to(torch.int32)
    pos = rows >= 0
    if cfg["op"] == "gather":
        src = torch.randn((cfg["n_other"], lds), generator=g).to(dt).to(DEV)
        dbuf = Guarded(R * ldd, dt)
        ops.gather_rows(src, lds, rows32, R, H, dbuf.t, ldd)
        dst = dbuf.t.view(R, ldd)
        assert dbuf.guards_untouched(), info
        assert _same_bits(dst[pos][:, :H], src[rows[pos]][:, :H]), info
        assert bool((_bits(dst[~pos][:, :H]) == 0).all()), info                          # "no such row": zeros, +0
        assert bool(torch.isnan(dst[:, H:].float()).all()), info
        return
    src = torch.randn((R, lds), generator=g).to(dt).to(DEV)
    dst0 = torch.randn((cfg["n_other"], ldd), generator=g).to(dt).to(DEV)
    dbuf = Guarded(cfg["n_other"] * ldd, dt)
    dbuf.t.copy_(dst0.view(-1))
    accumulate = cfg["op"] == "scatter_acc"
    ops.scatter_rows(src, lds, rows32, R, H, dbuf.t, ldd, accumulate=accumulate)
    dst = dbuf.t.view(cfg["n_other"], ldd)
    want = dst0.clone()
    want[rows[pos], :H] = (dst0[rows[pos], :H].float() + src[pos][:, :H].float()).to(dt) if accumulate else src[pos][:, :H]
    assert dbuf.guards_untouched(), info
    assert _same_bits(dst, want), info               # the written rows, and every other row and the padding columns untouched


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.cs_cases(), ids=lambda c: f"{c['seed']}-{c['dt']}-M{c['M']}-N{c['N']}")
def test_colsum_random_configurations(cfg):
    M, N, ldx, dt = cfg["M"], cfg["N"], cfg["ldx"], C.DT[cfg["dt"]]
    info = dict(cfg, branches=C.cs_branches(cfg), plan=C.cs_plan(cfg))
    gdev = DEV if M * ldx > C.CS_MAX_ELEMS else "cpu"           # drawn on the CPU, except the few cases of more than 8M elements
    g = torch.Generator(device=gdev).manual_seed(cfg["seed"])
    flat = torch.empty(cfg["off"] + M * ldx, dtype=dt, device=DEV)
    flat.copy_(torch.randn(flat.shape, generator=g, device=gdev, dtype=torch.float32) + 0.25)
    x = flat[cfg["off"]:].view(M, ldx)
    before = flat.clone()
    out = Guarded(N, torch.float32)
    start = torch.randn((N,), generator=torch.Generator().manual_seed(cfg["seed"])).to(DEV)
    out.t.copy_(start)
    us = cfg["unscale"]
    us_t = torch.tensor([us], dtype=torch.float32, device=DEV) if us is not None else None
    ops.colsum(x, ldx, M, N, out.t, accumulate=bool(cfg["accumulate"]), unscale=us_t)
    f = 1.0 if us is None else us
    base = start.double() if cfg["accumulate"] else torch.zeros(N, dtype=torch.float64, device=DEV)
    want = base + f * x[:, :N].sum(0, dtype=torch.float64)
    mag = base.abs() + f * x[:, :N].abs().sum(0, dtype=torch.float64)
    ok, worst = _within(out.t, want, C.sum_bound(M + 2, mag))
    print(f"colsum {cfg['seed']} {info['branches']} error / bound {worst:.3f}")
    assert out.guards_untouched() and torch.equal(_bits(flat), _bits(before)), info
    assert ok, (info, worst)


@pytest.mark.parametrize("cfg", C.cp_cases(), ids=lambda c: f"{c['seed']}-P{c['P']}-N{c['N']}")
def test_colsum_partials_random_configurations(cfg):
    P, N, ld = cfg["P"], cfg["N"], cfg["ld"]
    info = dict(cfg, branches=C.cp_branches(cfg))
    g = torch.Generator().manual_seed(cfg["seed"])
    part = torch.randn((P, ld), generator=g).to(DEV)
    part[:, N:] = 1e30                                   # padding columns: never part of a sum
    out = Guarded(N, torch.float32)
    start = torch.randn((N,), generator=g).to(DEV)
    out.t.copy_(start)
    us = cfg["unscale"]
    us_t = torch.tensor([us], dtype=torch.float32, device=DEV) if us is not None else None
    ops.colsum_partials(part, P, ld, N, out.t, unscale=us_t)
    f = 1.0 if us is None else us
    want = start.double() + f * part[:, :N].double().sum(0)
    mag = start.double().abs() + f * part[:, :N].double().abs().sum(0)
    ok, worst = _within(out.t, want, C.sum_bound(P + 2, mag))
    assert out.guards_untouched(), info
    assert ok, (info, worst)


# =====================================================================================================================
def _cast(cfg, info):
    n, src, dst = cfg["n"], cfg["src"], C.DT[cfg["dst"]]
    x_c = C.cast_input(n, src, cfg["seed"])
    x = x_c.to(DEV)
    out = Guarded(n, dst)
    ops.cast(x, out.t, n)
    want = x_c.to(dst)                                   # torch on the CPU: IEEE round-to-nearest-even
    assert out.guards_untouched(), info
    got = out.t.cpu()
    bad = ~((_bits(got) == _bits(want)) | (torch.isnan(got) & torch.isnan(want)))
    assert not bool(bad.any()), (info, "first mismatches (index, input, got, want)",
                                 [(int(i), float(x_c[i]), float(got[i]), float(want[i])) for i in bad.nonzero().flatten()[:8]])


def _cast2d(cfg, info):
    rows, cols, lds, ldd = cfg["rows"], cfg["cols"], cfg["lds"], cfg["ldd"]
    sdt, ddt = C.DT[cfg["src"]], C.DT[cfg["dst"]]
    sp = C.cast_input(min(rows * lds, 4096), cfg["src"], cfg["seed"])
    src_c = (torch.randn((rows * lds,), generator=torch.Generator().manual_seed(cfg["seed"])) * 3.0).to(sdt)
    src_c[:sp.numel()] = sp
    src_c[-sp.numel():] = sp                                # the last rows (the second launch, if any) carry the specials too
    src_c = src_c.view(rows, lds)
    out = Guarded(rows * ldd, ddt)
    ops.cast2d(src_c.to(DEV), lds, out.t, ldd, rows, cols)
    got = out.t.view(rows, ldd)
    assert out.guards_untouched(), info
    assert _same_values(got[:, :cols].cpu(), src_c[:, :cols].to(ddt)), info
    assert bool((_bits(got[:, cols:]) == 0).all()), info                                  # zero-filled by the ABI


def _add(cfg, info):
    n, dt = cfg["n"], C.DT[cfg["dt"]]
    g = torch.Generator().manual_seed(cfg["seed"])
    a, b = (torch.randn((n,), generator=g) * 2.0).to(dt).to(DEV), (torch.randn((n,), generator=g) * 2.0).to(dt).to(DEV)
    out = Guarded(n, dt)
    ops.add(a, b, out.t, n)
    assert out.guards_untouched(), info
    assert _same_bits(out.t, (a.float() + b.float()).to(dt)), info


def _dact(cfg, info):
    n, dt, mode = cfg["n"], C.DT[cfg["dt"]], cfg["mode"]
    g = torch.Generator().manual_seed(cfg["seed"])
    dy = torch.randn((n,), generator=g).to(dt).to(DEV)
    z = (torch.randn((n,), generator=g) * 1.5).to(dt)
    z = (torch.tanh(z.float()).to(dt) if mode == 1 else z).to(DEV)         # modes 1 and 2 read the activation's OUTPUT
    if mode == 2:
        z[::7] = 0.0
        z[3::11] = -0.0
    out = Guarded(n, dt)
    ops.dact(mode, dy, z, out.t, n)
    assert out.guards_untouched(), info
    d64, z64 = dy.double(), z.double()
    if mode == 2:                                                            # a select: exact
        assert _same_bits(out.t, torch.where(z > 0, dy, torch.zeros_like(dy))), info
        return
    want = (d64 * C.dgelu64(z64) if mode == 0 else d64 * (1.0 - z64 * z64)).view(1, n)
    if cfg["dt"] == C.F32:
        err = _rowrel(out.t.view(1, n), want)
        assert err < DACT_TOL, (info, err)
    else:
        ok, worst = _within(out.t.view(1, n), want, C.out16_bound(want, cfg["dt"], DACT_TOL))
        assert ok, (info, worst)


def _transpose(cfg, info):
    rows, cols, dt = cfg["rows"], cfg["cols"], C.DT[cfg["dt"]]
    x = torch.randn((rows, cols + 3), generator=torch.Generator().manual_seed(cfg["seed"])).to(dt).to(DEV)
    out = Guarded(cols * (rows + 5), dt)
    ops.transpose(x, out.t, rows, cols, lds=cols + 3, ldd=rows + 5)
    y = out.t.view(cols, rows + 5)
    assert out.guards_untouched(), info
    assert _same_bits(y[:, :rows], x[:, :cols].t()) and bool(torch.isnan(y[:, rows:].float()).all()), info


@pytest.mark.parametrize("cfg", C.ew_cases(), ids=lambda c: "-".join(str(c[k]) for k in ("seed", "op", "src", "dst", "dt", "mode", "n", "rows", "ldd") if k in c))
def test_elementwise_configurations(cfg):
    info = dict(cfg, branches=C.ew_branches(cfg))
    {"cast": _cast, "cast2d": _cast2d, "add": _add, "dact": _dact, "transpose": _transpose}[cfg["op"]](cfg, info)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.nf_cases(), ids=lambda c: f"{c['seed']}-n{c['n']}-k{c['k']}")
def test_count_nonfinite_configurations(cfg):
    info = dict(cfg, branches=C.nf_branches(cfg), positions=C.nf_positions(cfg))
    x_c, k = C.nf_input(cfg)
    assert k == cfg["k"] and int((~torch.isfinite(x_c)).sum()) == k, info
    x = x_c.to(DEV)
    assert torch.equal(_bits(x.cpu()), _bits(x_c)), info               # the copy keeps NaN payloads
    counter = Guarded(1, torch.float32, fill=float(cfg["start"]))
    ops.count_nonfinite(x, counter.t)
    assert counter.guards_untouched(), info
    assert float(counter.t[0]) == float(cfg["start"] + k), (info, float(counter.t[0]))


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.aw_cases(), ids=lambda c: f"{c['seed']}-n{c['n']}-{c['shadows']}-{c['state']}")
def test_adamw_three_steps(cfg):
    n, hy, wd = cfg["n"], C.AW_HYPER, cfg["wd"]
    info = dict(cfg, branches=C.aw_branches(cfg))
    gdev = DEV if n > (1 << 20) else "cpu"                              # drawn on the CPU, except the 4M-element cases
    g = torch.Generator(device=gdev).manual_seed(cfg["seed"])
    p0 = torch.randn((n,), generator=g, device=gdev).to(DEV)
    scale_up = 1.0 / cfg["grad_scale"]                                  # gradients arrive multiplied by the loss scale
    grads = [(torch.randn((n,), generator=g, device=gdev) * (0.5 + s) * scale_up).to(DEV) for s in range(3)]
    p, m, v = Guarded(n, torch.float32), Guarded(n, torch.float32, fill=0.0), Guarded(n, torch.float32, fill=0.0)
    p.t.copy_(p0)
    sb = Guarded(n, torch.bfloat16) if cfg["shadows"] in ("both", "bf16") else None
    sh = Guarded(n, torch.float16) if cfg["shadows"] in ("both", "f16") else None
    st = torch.zeros(8, dtype=torch.float32, device=DEV) if cfg["state"] != "none" else None
    if cfg["state"] == "skip":
        st[3] = 1.0
    ref = C.hf_adamw_reference(p0, grads, wd=wd, correct_bias=cfg["correct_bias"], grad_scale=cfg["grad_scale"], **hy)
    gmax = torch.zeros(n, dtype=torch.float64, device=DEV)
    for t in range(1, 4):
        if cfg["state"] == "live":
            st[4] = float(t)                                             # t comes from the device state, the host's step is ignored
        ops.adamw_step(p.t, grads[t - 1], m.t, v.t, sb.t if sb else None, n, hy["lr"], hy["b1"], hy["b2"], hy["eps"], wd,
                       t if st is None else 77, correct_bias=bool(cfg["correct_bias"]), grad_scale=cfg["grad_scale"],
                       shadow_f16=sh.t if sh else None, scaler_state=st)
        for b in (p, m, v, sb, sh):
            assert b is None or b.guards_untouched(), (info, t)
        if cfg["state"] == "skip":                                       # an overflowed step moves nothing
            assert _same_bits(p.t, p0) and bool((_bits(m.t) == 0).all()) and bool((_bits(v.t) == 0).all()), (info, t)
            assert (sb is None or bool(torch.isnan(sb.t.float()).all())) and (sh is None or bool(torch.isnan(sh.t.float()).all())), (info, t)
        else:
            gmax = torch.maximum(gmax, (grads[t - 1].double() * C.f32r(cfg["grad_scale"])).abs())
            bp, bm, bv = C.aw_bounds(ref[t - 1][0], gmax, hy["lr"], t)
            for name, got, want, bound in (("p", p.t, ref[t - 1][0], bp), ("m", m.t, ref[t - 1][1], bm), ("v", v.t, ref[t - 1][2], bv)):
                ok, worst = _within(got, want, bound)
                assert ok, (info, t, name, worst)
            assert sb is None or _same_bits(sb.t, p.t.to(torch.bfloat16)), (info, t)
            assert sh is None or _same_bits(sh.t, p.t.to(torch.float16)), (info, t)


# =====================================================================================================================
@pytest.mark.parametrize("cfg", C.dm_cases(), ids=lambda c: f"n{c['n']}-p{c['p']}")
def test_dropout_mask_properties(cfg):
    n, p = cfg["n"], cfg["p"]
    info = dict(cfg, branches=C.dm_branches(cfg))
    thr = C.dm_threshold(p)
    masks = {}
    for key in C.DM_KEYS:
        keep, scale = ops.dropout_mask(p, key, n, DEV)
        again, _ = ops.dropout_mask(p, key, n, DEV)
        longer, _ = ops.dropout_mask(p, key, n + 1, DEV)
        assert scale == C.f32r(65536.0 / (65536.0 - round(p * 65536))) and thr == round(p * 65536), (info, scale)
        assert keep.dtype == torch.uint8 and bool((keep <= 1).all()), info
        assert torch.equal(keep, again), info                            # the same key twice: the same bits
        assert torch.equal(keep, longer[:n]), info                       # prefix property
        # pair structure: one hash per pair of elements, element i reads half i & 1 (restated with numpy)
        assert np.array_equal(keep.cpu().numpy(), C.dm_restated(p, key, n)), info
        if p == 0:
            assert bool(keep.all()) and scale == 1.0, info
        if n >= 65536:
            q = 1.0 - thr / 65536.0
            rate = int(keep.sum(dtype=torch.int64)) / n              # an exact count: a mean of two million ones in floating point is not 1
            sigma = np.sqrt(q * (1.0 - q) / n)
            print(f"mask n={n} p={p} key={key:#x}: keep rate {rate:.6f}, expected {q:.6f}, sigma {sigma:.2e}")
            assert abs(rate - q) <= 5.0 * sigma, (info, rate, q)
            for half in (0, 1):                                          # both halves of the hash word
                part = keep[half::2]
                hr = int(part.sum(dtype=torch.int64)) / part.numel()
                assert abs(hr - q) <= 5.0 * np.sqrt(q * (1.0 - q) / part.numel()), (info, half, hr)
        masks[key] = keep
    if n >= 65536 and p > 0:
        # two keys are independent: of the positions one key drops, the other drops a fraction thr / 65536 (half of them at p = 0.5)
        a, b = (masks[k].bool() for k in C.DM_KEYS)
        dropped = ~a
        nd = int(dropped.sum())
        qd = thr / 65536.0
        frac = int((~b[dropped]).sum(dtype=torch.int64)) / nd
        assert abs(frac - qd) <= 5.0 * np.sqrt(qd * (1.0 - qd) / nd), (info, frac, qd, nd)
