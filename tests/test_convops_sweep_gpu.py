"""Sweep of the region encoder's support kernels (csrc/mv_conv.hip: mv_nchw_to_nhwc, mv_im2col, mv_col_stats, mv_bn_finalize,
mv_bn_act, mv_maxpool3x3s2) over the cases of tests/convops_cases.py, against float64 references with one bound per output element.
convops_cases.py derives the bounds; tests/test_convops_cases_cpu.py shows that they let an honest f32 computation through and catch
each planted defect, and proves which launcher branch every case takes.  Every case runs: nothing here may drop one.

Per case: the output sits inside a NaN-filled buffer, with guard elements in front and guard rows behind; leading dimensions carry
NaN padding where the ABI has one (ldx; the columns kh*kw*C..ldk-1 of mv_im2col belong to the output and must come back +0);
everything outside the logical extent must come back bit-identical, the inputs too.  References are computed on the device.
* data movement (nchw_to_nhwc, im2col, maxpool): bit-exact;
* col_stats: bit-exact on the exactly summable inputs, 2 rows 2^-24 sum|terms| on the Gaussian ones;
* bn_finalize, bn_act: the bounds derived from the arithmetic as written (convops_cases.fin_bounds, act_reference).
The assertion messages carry the cfg dict, which reproduces the case."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import convops_cases as C                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Out:
    """rows x cols of `dtype` inside a NaN-filled device buffer: C.GUARD + off elements in front, C.GUARD_ROWS rows behind"""

    def __init__(self, rows, cols, dtype, off=0, fill=C.NAN):
        self.rows, self.cols, self.off = rows, cols, C.GUARD + off
        self.flat = torch.full((self.off + (rows + C.GUARD_ROWS) * cols,), fill, dtype=dtype, device=DEV)
        self.before = self.flat.clone()
        self.t = self.flat[self.off:self.off + rows * cols].view(rows, cols)

    def expect(self, ref):
        """the whole buffer as it has to look if the logical extent holds `ref` and nothing else was touched"""
        e = self.before.clone()
        e[self.off:self.off + self.rows * self.cols] = ref.reshape(-1)
        return e

    def exactly(self, ref):
        return torch.equal(C.bits(self.flat), C.bits(self.expect(ref)))

    def guards_untouched(self):
        return self.exactly(self.t)


def _mismatch(out, ref):
    """where the logical extent differs from the reference, for the assertion message"""
    bad = (C.bits(out.t) != C.bits(ref)).nonzero()
    if bad.numel() == 0:
        return "logical extent equal; a guard element changed"
    r, c = bad[0].tolist()
    return "%d elements differ, first at (%d, %d): got %r, want %r" % (bad.shape[0], r, c, float(out.t[r, c]), float(ref[r, c]))


@pytest.mark.parametrize("cfg", C.nhwc_cases(), ids=C.case_id)
def test_nchw_to_nhwc_cases(cfg):
    info = dict(cfg, branches=C.nhwc_branches(cfg))
    x = C.nhwc_inputs(cfg).to(DEV)
    x0 = x.clone()
    B, Cc, H, W, Cp = cfg["B"], cfg["C"], cfg["H"], cfg["W"], cfg["Cp"]
    out = Out(B * H * W, Cp, C.DT[cfg["dt"]])
    ops.nchw_to_nhwc(x, out.t, B, Cc, H, W, Cp)
    ref = C.nhwc_reference(x0, cfg)
    print(f"{C.case_id(cfg)}: bit-exact check over {ref.numel()} elements")
    assert out.exactly(ref), (_mismatch(out, ref), info)
    assert torch.equal(x, x0), info


@pytest.mark.parametrize("cfg", C.im2col_cases(), ids=C.case_id)
def test_im2col_cases(cfg):
    info = dict(cfg, plan=C.im2col_plan(cfg)[:3], branches=C.im2col_branches(cfg))
    x = C.im2col_inputs(cfg).to(DEV)
    x0 = x.clone()
    Ho, Wo, rows, kc = C.im2col_shape(cfg)
    out = Out(rows, cfg["ldk"], x.dtype, off=cfg["dst_off"])
    assert (out.t.data_ptr() % 16 == 0) == ("VEC4:misaligned" not in info["branches"]) and x.data_ptr() % 16 == 0, info
    ops.im2col(x, out.t, cfg["B"], cfg["H"], cfg["W"], cfg["C"], cfg["kh"], cfg["kw"], cfg["stride"], cfg["pad"], cfg["ldk"])
    ref = C.im2col_reference(x0, cfg)
    print(f"{C.case_id(cfg)}: {info['plan'][0]}, bit-exact check over {rows} x {cfg['ldk']}")
    assert out.exactly(ref), (_mismatch(out, ref), info)                     # the tail columns: +0, bit for bit
    assert torch.equal(C.bits(x), C.bits(x0)), info


@pytest.mark.parametrize("cfg", C.pool_cases(), ids=C.case_id)
def test_maxpool3x3s2_cases(cfg):
    info = dict(cfg, branches=C.pool_branches(cfg))
    x = C.pool_inputs(cfg).to(DEV)
    x0 = x.clone()
    Ho, Wo, rows = C.pool_shape(cfg)
    out = Out(rows, cfg["C"], x.dtype)
    ops.maxpool3x3s2(x, out.t, cfg["B"], cfg["H"], cfg["W"], cfg["C"])
    ref = C.pool_reference(x0, cfg)
    print(f"{C.case_id(cfg)}: bit-exact check over {rows} x {cfg['C']}")
    assert out.exactly(ref), (_mismatch(out, ref), info)
    assert torch.equal(C.bits(x), C.bits(x0)), info


@pytest.mark.parametrize("cfg", C.stats_cases(), ids=C.case_id)
def test_col_stats_cases(cfg):
    info = dict(cfg, plan=C.stats_plan(cfg["rows"]), branches=C.stats_branches(cfg))
    rows, Cc, ldx = cfg["rows"], cfg["C"], cfg["ldx"]
    xin = Out(rows, ldx, C.DT[cfg["dt"]])                                     # the input gets guards too: nothing reads past it unnoticed
    xin.t.copy_(C.stats_inputs(cfg).to(DEV))
    x0 = xin.flat.clone()
    st = Out(2, Cc, torch.float32)                                            # NaN-filled: the launcher has to clear it
    ops.col_stats(xin.t, ldx, rows, Cc, st.t)
    ref, bound = C.stats_reference(xin.t, cfg)
    ok, worst = C.within(st.t, ref, bound)
    print(f"{C.case_id(cfg)}: {'exact' if cfg['kind'] == 'int' else 'error / bound %.4f' % worst}")
    assert st.guards_untouched(), info
    assert ok, ("error / bound = %.3g" % worst, info, st.t, ref)
    assert torch.equal(C.bits(xin.flat), C.bits(x0)), info


@pytest.mark.parametrize("cfg", C.fin_cases(), ids=C.case_id)
def test_bn_finalize_cases(cfg):
    info = dict(cfg, branches=C.fin_branches(cfg))
    Cc = cfg["C"]
    stats_c, rm_c, rv_c = C.fin_inputs(cfg)
    stats, rm0, rv0 = stats_c.to(DEV), rm_c.to(DEV), rv_c.to(DEV)
    s0 = stats.clone()
    mean, rstd, rm, rv = (Out(1, Cc, torch.float32) for _ in range(4))
    rm.t.copy_(rm0.view(1, Cc))                                               # the running buffers start from non-trivial values
    rv.t.copy_(rv0.view(1, Cc))
    held = (rm.flat.clone(), rv.flat.clone())
    run = cfg["running"]
    ops.bn_finalize(stats, Cc, cfg["rows"], cfg["eps"], cfg["momentum"], mean.t, rstd.t, rm.t if run else None, rv.t if run else None)
    ref = C.fin_reference(stats, rm0, rv0, cfg)
    bnd = C.fin_bounds(ref, rm0, rv0, cfg)
    res = {"mean": C.within(mean.t[0], ref["mean"], bnd["mean"]), "rstd": C.interval_ratio(rstd.t[0], ref["rstd"], *bnd["rstd"])}
    if run:
        res["run_mean"] = C.within(rm.t[0], ref["run_mean"], bnd["run_mean"])
        res["run_var"] = C.within(rv.t[0], ref["run_var"], bnd["run_var"])
    print(f"{C.case_id(cfg)}: error / bound " + " ".join("%s %.4f" % (k, r) for k, (_, r) in res.items()))
    for o in (mean, rstd, rm, rv):
        assert o.guards_untouched(), info
    for k, (ok, r) in res.items():
        assert ok, (k, "error / bound = %.3g" % r, info)
    if not run:                                                               # pointers None: the buffers come back as they were
        assert torch.equal(C.bits(rm.flat), C.bits(held[0])) and torch.equal(C.bits(rv.flat), C.bits(held[1])), info
    exact0 = 1.0 / C.f32r(cfg["eps"]) ** 0.5                                 # column 0: the variance comes out exactly 0, three roundings remain
    assert abs(float(rstd.t[0, 0]) - exact0) <= 3.0 * C.U32 * exact0, info
    assert torch.equal(stats, s0), info


@pytest.mark.parametrize("cfg", C.act_cases(), ids=C.case_id)
def test_bn_act_cases(cfg):
    info = dict(cfg, branches=C.act_branches(cfg))
    rows, Cc = cfg["rows"], cfg["C"]
    x, mean, rstd, gamma, beta, res = (t.to(DEV) if t is not None else None for t in C.act_inputs(cfg))
    held = [t.clone() for t in (x, mean, rstd, gamma, beta)] + ([res.clone()] if res is not None else [])
    out = Out(rows, Cc, C.DT[cfg["ydt"]])
    ops.bn_act(x, mean, rstd, gamma, beta, out.t, rows, Cc, residual=res, relu=cfg["relu"])
    ref, bound = C.act_reference(x, mean, rstd, gamma, beta, res, cfg)
    ok, worst = C.within(out.t, ref, bound)
    print(f"{C.case_id(cfg)}: error / bound {worst:.4f}")
    assert out.guards_untouched(), info
    assert ok, ("error / bound = %.3g" % worst, info)
    if cfg["relu"]:
        assert bool((out.t >= 0).all()), info
    for a, b in zip([x, mean, rstd, gamma, beta] + ([res] if res is not None else []), held):
        assert torch.equal(C.bits(a), C.bits(b)), info


def test_batch_statistics_conditioning():
    """mv_col_stats + mv_bn_finalize on one 112 x 112 stem map (12544 rows, 64 columns, f32): N(mu, 1) columns for mu in
    0, 1, 3, 10, 30, 100 and one constant column, against the two-pass statistics in float64.  Asserted: the bound of the single-pass
    formula, |dvar| <= 2 rows 2^-24 (E[x^2] + mean^2) + the finalize terms, carried to rstd through var + eps (with the clamp at 0).
    Printed alongside: what F.batch_norm in f32 on the CPU makes of the same input.  DESIGN.md records the figures."""
    x_c, mu = C.cond_inputs()
    x = x_c.to(DEV)
    st = torch.full((2, C.COND_C), C.NAN, dtype=torch.float32, device=DEV)
    mean = torch.full((C.COND_C,), C.NAN, dtype=torch.float32, device=DEV)
    rstd = mean.clone()
    ops.col_stats(x, C.COND_C, C.COND_ROWS, C.COND_C, st)
    ops.bn_finalize(st, C.COND_C, C.COND_ROWS, C.COND_EPS, 0.1, mean, rstd)
    ref = {k: (tuple(t.cpu() for t in v) if isinstance(v, tuple) else v.cpu()) for k, v in C.cond_reference(x).items()}
    t_mean, t_rstd = C.cond_torch_f32(x_c)
    mean, rstd = mean.cpu().double(), rstd.cpu().double()
    lo, hi = ref["rstd_iv"]
    print("\n      mu |  kernel |mean err|  torch f32 |  kernel rstd rel err  torch f32   ratio | rstd bound (rel, lower / upper side) | var bound")
    groups = [(float(m), (mu == m).nonzero().view(-1)) for m in C.COND_MU] + [(None, torch.tensor([C.COND_C - 1]))]
    for m, idx in groups:
        k_m, t_m = (mean - ref["mean"]).abs()[idx].max(), (t_mean - ref["mean"]).abs()[idx].max()
        k_r, t_r = ((rstd - ref["rstd"]).abs() / ref["rstd"])[idx].max(), ((t_rstd - ref["rstd"]).abs() / ref["rstd"])[idx].max()
        b_lo, b_hi = ((ref["rstd"] - lo) / ref["rstd"])[idx].min(), ((hi - ref["rstd"]) / ref["rstd"])[idx].min()
        print("%8s | %.3e        %.3e  | %.3e             %.3e  %8.1f | %.3e / %.3e              | %.3e"
              % ("const" if m is None else "%g" % m, k_m, t_m, k_r, t_r, float(k_r / max(float(t_r), 1e-300)), b_lo, b_hi, ref["dvar"][idx].min()))
    ok_m, r_m = C.within(mean, ref["mean"], ref["dmean"])
    ok_r, r_r = C.interval_ratio(rstd, ref["rstd"], lo, hi)
    print("worst error / bound: mean %.4f rstd %.4f" % (r_m, r_r))
    assert ok_m, ("mean: error / bound = %.3g" % r_m, mean, ref["mean"])
    assert ok_r, ("rstd: error / bound = %.3g" % r_r, rstd, ref["rstd"])
