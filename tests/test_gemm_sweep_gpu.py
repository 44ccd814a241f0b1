"""Sweep of the GEMM kernels (mv_gemm, mv_conv2d) over the cases of tests/gemm_cases.py: every kernel family and variant, every route
of the automatic tile choice, the three bodies of the split-K reduce, every epilogue on each of its store paths, against float64
references with one bound per output element (gemm_cases.py derives them; tests/test_gemm_cases_cpu.py shows that they let an honest
f32 computation through and catch each planted defect, and proves which branch every case takes).

Per case: the bound element-wise, finiteness, the guard rows and columns of every output bit-identical, C3 bit-equal to C re-encoded
where both come from one f32 value, C2, and colsum_part (its rows, and folded with mv_colsum_partials).  Every test sets its knobs and
restores them in `finally`."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import _lib as L             # noqa: E402
from medvill_amd import hip_ops as ops        # noqa: E402

import gemm_cases as G                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KNOBS = ("impl", "gemm_force", "gemm_nj", "gemm_dbg", "gemm_rounds", "persistent_cus")
DEVICE_REFERENCE_ABOVE = 1 << 31              # M * N * K from which the float64 reference is computed on the device


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Knobs:
    """the case's kernel-forcing knobs, put back as they were on the way out"""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        self.saved = {k: L.get_knob(k) for k in KNOBS}
        c = self.cfg
        ops.set_impl(c.get("impl", 0))
        ops.set_gemm_variant(c.get("force", 0), c.get("nj", 0))
        ops.set_gemm_rounds(c.get("rounds", 1))
        ops.set_persistent_cus(c.get("pcus", 0))

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            L.set_knob(k, v)
        return False


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class _Out:
    """an output of M x N inside a poisoned buffer: `off` elements in front, leading dimension ld, guard rows behind"""

    def __init__(self, M, N, ld, off, dtype, init=None, guard_rows=G.GUARD_ROWS):
        x = init if init is not None else torch.full((M, N), NAN, dtype=dtype)
        flat, _ = G.place(x.to(dtype), ld, off, guard_rows)
        self.flat = flat.to(DEV)
        self.before = self.flat.clone()
        self.win = self.flat[off:].view(M + guard_rows, ld)
        self.M, self.N, self.off, self.ld = M, N, off, ld

    def got(self):
        return self.win[:self.M, :self.N]

    def restore(self):
        self.flat.copy_(self.before)

    def guards_untouched(self):
        a, b = self.flat.clone(), self.before.clone()
        for t in (a, b):
            t[self.off:].view(-1, self.ld)[:self.M, :self.N] = 0
        return torch.equal(_bits(a), _bits(b))


def _check(name, got, ref, bound, info, figures):
    ok, worst = G.within(got, ref.to(got.device), bound.to(got.device))
    figures.append("%s %.3f" % (name, worst))
    assert ok, (name, "error / bound = %.3g" % worst, info)


def _run_gemm(cfg):
    n_cu = _n_cu()
    pl = G.plan(cfg, n_cu)
    t = G.gemm_inputs(cfg, n_cu)
    fl = G.flags(cfg)
    M, N, K, epi = cfg["M"], cfg["N"], cfg["K"], cfg["epi"]
    info = (G.case_id(cfg), pl["kernel"], "slabs=%d" % pl["slabs"], pl["reduce"], cfg)
    A, B = t["A"].to(DEV), t["B"].to(DEV)
    bias = r = None
    if epi in G.NEED_BIAS:
        bflat, _ = G.place(t["bias"].view(1, N), N, cfg["bias_off"])
        bias = bflat.to(DEV)[cfg["bias_off"]:]
    if epi in G.NEED_R:
        rflat, _ = G.place(t["R"], fl["ldr"], cfg["r_off"])
        r = rflat.to(DEV)[cfg["r_off"]:].view(M, fl["ldr"])
    cdt = G.DT[cfg["cdt"]]
    C = _Out(M, N, fl["ldc"], cfg["c_off"], cdt, t["C0"])
    C2 = _Out(M, N, fl["ldc2"], cfg["c2_off"], cdt) if epi in G.NEED_C2 else None
    C3 = _Out(M, N, fl["ldc3"], cfg["c3_off"], G.DT[cfg["c3dt"]]) if cfg["c3dt"] else None
    wsf = G.ws_floats(cfg, n_cu)
    ws = torch.full((wsf,), NAN, dtype=torch.float32, device=DEV) if wsf else None
    alpha = torch.tensor([cfg["alpha"]], dtype=torch.float32, device=DEV) if cfg["alpha"] is not None else None
    P = 2 * G.cdiv(M, 256)
    part = _Out(P, N, N, 0, torch.float32, guard_rows=1) if cfg["csum"] else None
    # what the library says it would like as workspace is what the restated route wishes for
    assert ops.gemm_workspace_bytes(G.DT[cfg["dt"]], cfg["ta"], cfg["tb"], M, N, K) == G.workspace_bytes(cfg, n_cu), info

    def launch():
        ops.gemm(A, B, C.win, ta=bool(cfg["ta"]), tb=bool(cfg["tb"]), M=M, N=N, K=K, lda=t["lda"], ldb=t["ldb"], ldc=fl["ldc"], bias=bias, epi=epi,
                 r=r, ldr=fl["ldr"], c2=C2.win if C2 else None, ldc2=fl["ldc2"], c3=C3.win if C3 else None, ldc3=fl["ldc3"], splitk=cfg["splitk"],
                 ws=ws, accumulate=bool(cfg["accumulate"]), p_drop=cfg["p_drop"], drop_key=cfg["drop_key"], alpha=alpha,
                 colsum_part=part.win if part else None)
    launch()
    if cfg["launches"] == 2:                     # a second launch into the same buffers must give the same bits
        first = C.got().clone()
        if cfg["accumulate"]:
            C.restore()
        launch()
        assert torch.equal(_bits(first), _bits(C.got())), ("the second launch differs from the first", info)
    torch.cuda.synchronize()
    ref = G.gemm_reference(cfg, t, pl, DEV if M * N * K >= DEVICE_REFERENCE_ABOVE else "cpu")
    figures = []
    try:
        _check("C", C.got(), *ref["C"], info, figures)
        assert C.guards_untouched(), ("C: guard rows / columns written", info)
        if C2:
            _check("C2", C2.got(), *ref["C2"], info, figures)
            assert C2.guards_untouched(), ("C2: guard rows / columns written", info)
        if C3:
            _check("C3", C3.got(), *ref["C3"], info, figures)
            assert C3.guards_untouched(), ("C3: guard rows / columns written", info)
            if cfg["cdt"] == G.F32 or cfg["cdt"] == cfg["c3dt"]:        # one f32 value, two encodings
                assert torch.equal(_bits(C3.got()), _bits(C.got().to(C3.got().dtype))), ("C3 is not C re-encoded", info)
        if part:
            _check("colsum_part", part.got(), *ref["csum"], info, figures)
            assert part.guards_untouched(), ("colsum_part: row past 2 * ceil(M / 256) written", info)
            folded = torch.zeros((N,), dtype=torch.float32, device=DEV)
            ops.colsum_partials(part.got(), P, N, N, folded)
            _check("colsum", folded.view(1, N), ref["colsum"][0].view(1, N), ref["colsum"][1].view(1, N), info, figures)
    finally:
        print("\n%s [%s, %d slab(s), %s]: error / bound %s" % (G.case_id(cfg), pl["kernel"], pl["slabs"], pl["reduce"], ", ".join(figures)))
    return pl


def _gemm_case(cfg):
    with _Knobs(cfg):
        return _run_gemm(cfg)


@pytest.mark.parametrize("cfg", G.small_cases(), ids=G.case_id)
def test_small(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.ring_cases(), ids=G.case_id)
def test_ring(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.pring_cases(), ids=G.case_id)
def test_pring_walk(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.valu_cases(), ids=G.case_id)
def test_valu(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.auto_cases(), ids=G.case_id)
def test_auto(cfg):
    """the automatic tile choice: the restated route, evaluated with THIS device's CU count, must name the route the census counted
    (gemm_cases.AUTO_TABLE); a device with another CU count fails here instead of sweeping something else"""
    want = G.AUTO_TABLE[cfg["seed"]][7]
    pl = G.plan(cfg, _n_cu())
    assert (pl["rule"], pl["kernel"], pl["slabs"]) == want, ("CU count %d: the case no longer takes its route" % _n_cu(), want, pl)
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.reduce_cases(), ids=G.case_id)
def test_reduce(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.workspace_cases(), ids=G.case_id)
def test_workspace(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.epi_cases(), ids=G.case_id)
def test_epi(cfg):
    _gemm_case(cfg)


@pytest.mark.parametrize("cfg", G.conv_cases(), ids=G.conv_id)
def test_conv(cfg):
    c = cfg
    with _Knobs(c):
        Ho, Wo, M, K = G.conv_dims(c)
        t = G.conv_inputs(c)
        x = t["x"].reshape(c["B"] * c["H"] * c["W"], c["C"]).to(DEV)
        w = t["w"].reshape(c["O"], K).to(DEV)
        y = _Out(M, c["O"], c["O"], 0, G.DT[c["cdt"]])
        bias = t["bias"].to(DEV) if c["epi"] != G.EPI_NONE else None
        r = t["R"].to(DEV) if c["rdt"] else None
        ops.conv2d(x, w, y.win, c["B"], c["H"], c["W"], c["C"], c["O"], c["k"], c["k"], c["s"], c["p"], bias=bias, epi=c["epi"], r=r)
        torch.cuda.synchronize()
        ref = G.conv_reference(c, t)
        figures = []
        try:
            _check("y", y.got(), *ref["C"], (G.conv_id(c), c), figures)
            assert y.guards_untouched(), ("y: guard rows written", c)
        finally:
            print("\n%s: error / bound %s" % (G.conv_id(c), ", ".join(figures)))


@pytest.mark.parametrize("force,nj", [(1, 0), (2, 14)])
def test_function_tolerances_hold(force, nj):
    """tanh and GELU as the epilogues evaluate them, on a product whose f32 value is exact (gemm_cases.function_grid): the figures
    gemm_cases.TANH_MEASURED / GELU_MEASURED were read from, printed again, against the constants made of them"""
    a, b, z = G.function_grid()
    M, N = z.shape
    cfg = dict(force=force, nj=nj)
    with _Knobs(cfg):
        A, B = a.to(DEV), b.to(DEV)
        zero = torch.zeros((N,), dtype=torch.float32, device=DEV)
        c = torch.full((M, N), NAN, dtype=torch.float32, device=DEV)
        c2 = torch.full((M, N), NAN, dtype=torch.float32, device=DEV)
        ops.gemm(A, B, c, M=M, N=N, K=8, bias=zero, epi=G.EPI_BIAS_TANH)
        tanh_err = float((c.double().cpu() - torch.tanh(z)).abs().max())
        ops.gemm(A, B, c, M=M, N=N, K=8, bias=zero, epi=G.EPI_BIAS_GELU, c2=c2)
        assert torch.equal(c2.double().cpu(), z), "the pre-activation of the grid is exact"
        gelu_err = float(((c.double().cpu() - G.gelu64(z)).abs() / (1 + z.abs())).max())
        ops.gemm(A, B, c, M=M, N=N, K=8, bias=zero, epi=G.EPI_BIAS_GELU_D, c2=c2)
        gelu_d_err = float(((c.double().cpu() - G.gelu64(z)).abs() / (1 + z.abs())).max())
        dgelu_err = float((c2.double().cpu() - G.dgelu64(z)).abs().max())
    print("\nmeasured on the exact grid (force=%d, nj=%d): tanh %.3g (constant %.3g), gelu %.3g and %.3g (constant %.3g, relative to 1 + |z|), "
          "gelu' %.3g (constant %.3g)" % (force, nj, tanh_err, G.TANH_TOL, gelu_err, gelu_d_err, G.GELU_TOL, dgelu_err, G.DACT_TOL))
    assert tanh_err <= G.TANH_TOL and max(gelu_err, gelu_d_err) <= G.GELU_TOL and dgelu_err <= G.DACT_TOL
