"""Sweep of the grouped weight-gradient launch (mv_gemm_grouped_tn) over the cases of tests/gemm_grouped_cases.py: the raster's
second row group and n0 > 0, all-split launches, tails that span problems with different kchunk, both bodies of the grouped reduction,
and one block walking many units of every kind, against float64 references with one bound per output element
(gemm_grouped_cases.py derives them; tests/test_gemm_grouped_cases_cpu.py shows that they let an honest f32 computation through and
catch each planted defect, and counts what every case reaches).

Per case: the header and the unit list of the table equal the restated plan, every element inside its bound and finite, every guard
element of C still NaN, a second launch (and a launch on another grid) bit-identical, and a single problem with nothing split
bit-identical to mv_gemm.  The operands' padding, the workspace and C are NaN before the launch."""
import ctypes
import time

import pytest
import torch

from medvill_amd import hip_ops as ops

import gemm_grouped_cases as GG

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DEVICE_REFERENCE_ABOVE = 1 << 28              # sum of No * Ko * rows from which the float64 products are formed on the device
_WORST = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Problem:
    """one problem on the device: operands in their NaN-padded storage, C in its poisoned buffer"""

    def __init__(self, p):
        self.p = p
        self.A, self.B = p["A"].to(DEV), p["B"].to(DEV)
        flat, _ = GG.c_buffer(p)
        self.before = flat.to(DEV)
        self.flat = self.before.clone()
        self.win = self.flat[p["c_off"]:].view(p["No"] + GG.GUARD_ROWS, p["ldc"])

    def entry(self):
        p = self.p
        return (self.A[:, p["a_col"]:], self.B, self.win, p["No"], p["Ko"], p["rows"], p["lda"], p["ldb"], p["ldc"])

    def got(self):
        return self.win[:self.p["No"], :self.p["Ko"]]

    def restore(self):
        self.flat.copy_(self.before)

    def guards_are_nan(self):
        g = self.flat.clone()
        g[self.p["c_off"]:].view(-1, self.p["ldc"])[:self.p["No"], :self.p["Ko"]] = NAN
        return bool(torch.isnan(g).all())


def _launch(c, probs, pcus):
    """plan for c["G"] blocks, launch under set_persistent_cus(pcus) -> the table"""
    ops.set_persistent_cus(pcus)
    t = ops.GroupedTN(DEV)
    t.set(GG.DT[c["dt"]], [q.entry() for q in probs], n_blocks=c["G"])
    wb = t.workspace_bytes()
    ws = torch.full((max(wb // 4, 1),), NAN, dtype=torch.float32, device=DEV)
    alpha = torch.tensor([c["alpha"]], dtype=torch.float32, device=DEV) if c["alpha"] is not None else None
    t.launch(ws=ws if wb else None, accumulate=bool(c["accumulate"]), alpha=alpha)
    torch.cuda.synchronize()
    return t


def _run(c):
    t0 = time.time()
    hdr, units = GG.group_plan(c["shapes"], c["G"])
    inputs = GG.group_inputs(c)
    probs = [_Problem(p) for p in inputs]
    info = (GG.case_id(c), (hdr["direct"], hdr["tail"], hdr["split"]), c)
    figures = []
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for pcus in c["pcus"]:          # the walk the census counted is this device's walk: another CU count fails here instead of sweeping something else
        assert GG.launch_blocks(c, pcus, n_cu) == GG.launch_blocks(c, pcus), ("CU count %d: the launch grid is not the census's" % n_cu, info)
    try:
        first = None
        for pcus in c["pcus"]:
            for rep in range(c["launches"]):
                for q in probs:
                    q.restore()
                t = _launch(c, probs, pcus)
                words = list((ctypes.c_int * 16).from_buffer(t.host))
                assert words[3:8] == [c["G"], hdr["units"], hdr["direct"], hdr["tail"], hdr["split"]], ("header", words[3:8], info)
                assert t.workspace_bytes() == GG.workspace_bytes(hdr), info
                assert t.units() == units, ("the table's units are not the restated plan's", info)
                bits = [_bits(q.got()).clone() for q in probs]
                if first is None:
                    first = bits
                else:                                                   # the same plan, launched again or on another grid
                    for i, (x, y) in enumerate(zip(first, bits)):
                        assert torch.equal(x, y), ("problem %d: launch (pcus=%d, repeat %d) differs from the first" % (i, pcus, rep), info)
        big = sum(No * Ko * rows for No, Ko, rows in c["shapes"]) >= DEVICE_REFERENCE_ABOVE
        ref = GG.group_reference(c, inputs, DEV if big else "cpu")
        for i, (q, (r, bound)) in enumerate(zip(probs, ref)):
            ok, worst = GG.within(q.got().cpu(), r, bound)
            figures.append(worst)
            assert ok, ("problem %d %s: error / bound = %.3g" % (i, c["shapes"][i], worst), info)
            assert q.guards_are_nan(), ("problem %d: a guard element of C was written" % i, info)
        if c["single"] and hdr["tail"] == 0:                            # one problem, nothing split: the bits of an unsplit mv_gemm
            q, p = probs[0], inputs[0]
            mine = _bits(q.got()).clone()
            q.restore()
            alpha = torch.tensor([c["alpha"]], dtype=torch.float32, device=DEV) if c["alpha"] is not None else None
            ops.gemm(q.A[:, p["a_col"]:], q.B, q.win, ta=True, tb=True, M=p["No"], N=p["Ko"], K=p["rows"], lda=p["lda"], ldb=p["ldb"], ldc=p["ldc"],
                     splitk=1, alpha=alpha, accumulate=bool(c["accumulate"]))
            torch.cuda.synchronize()
            assert torch.equal(mine, _bits(q.got())), ("not the bits of mv_gemm(ta, tb, splitk=1)", info)
    finally:
        ops.set_persistent_cus(0)
        w = max(figures) if figures else float("nan")
        _WORST[c["fam"]] = max(_WORST.get(c["fam"], 0.0), w) if figures else _WORST.get(c["fam"], 0.0)
        print("\n%s plan %s: error / bound %.3f (largest of the %s family so far %.3f), %.2f s"
              % (GG.case_id(c), (hdr["direct"], hdr["tail"], hdr["split"]), w, c["fam"], _WORST[c["fam"]], time.time() - t0))


@pytest.mark.parametrize("cfg", GG.raster_cases(), ids=GG.case_id)
def test_raster(cfg):
    _run(cfg)


@pytest.mark.parametrize("cfg", GG.walk_cases(), ids=GG.case_id)
def test_walk(cfg):
    _run(cfg)


@pytest.mark.parametrize("cfg", GG.tail_cases(), ids=GG.case_id)
def test_tail(cfg):
    if cfg["shapes"] == GG.TAIL:
        h = GG.group_plan(cfg["shapes"], cfg["G"])[0]
        assert (h["direct"], h["tail"], h["split"]) == GG.TAIL_PLANS[GG.TAIL_G.index(cfg["G"])]
    _run(cfg)


@pytest.mark.parametrize("cfg", GG.layer_cases(), ids=GG.case_id)
def test_layer(cfg):
    """the engine's launch shapes: one layer on 256 blocks is the all-split plan (0, 108, 2) every training step runs"""
    h = GG.group_plan(cfg["shapes"], cfg["G"])[0]
    assert (h["direct"], h["tail"], h["split"]) in [want for _, _, want in GG.LAYER_PLANS]
    _run(cfg)


@pytest.mark.parametrize("cfg", GG.grid_cases(), ids=GG.case_id)
def test_grid(cfg):
    """one plan on two launch grids: bit-identical results, each inside the element bound"""
    _run(cfg)
