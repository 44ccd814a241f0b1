"""Census of the attention sweep (CPU).  tests/test_attn_fuzz_gpu.py is only worth its GPU time while its cases reach every tile path
of csrc/mv_attn*.hip; this file counts the paths from the dense masks, checks the constants the restatement relies on against the
sources, checks each fp64 reference against an independent formulation, and validates the bounds of tests/attn_cases.py with a torch
stand-in of the tile-wise algorithm: the honest stand-in stays below half of every bound on every case, and six deliberately wrong
ones each break a bound."""
import ast
import math
import os
import re
import sys
from collections import Counter

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import attn_cases as C                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "medvill.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_attn_fuzz_gpu.py")
MIN_HITS = 3


@pytest.fixture(scope="module")
def census():
    total, per_case = Counter(), []
    for c in C.all_cases():
        d = C.dispatch(c)
        per_case.append((c, d))
        total.update(set(d))
    return total, per_case


def test_every_named_branch_is_reached(census):
    total, _ = census
    for name in sorted(set(C.BRANCHES) | set(total)):
        print(f"    {name:32s} {total.get(name, 0):4d}{'' if name in C.BRANCHES else '   (not required)'}")
    short = {n: total.get(n, 0) for n in C.BRANCHES if total.get(n, 0) < MIN_HITS}
    assert not short, f"branches reached by fewer than {MIN_HITS} cases: {short}"


def test_every_value_set_length_dh_and_knob_is_drawn():
    cases = C.all_cases()
    mf = [c for c in cases if c["path"] == "mfma"]
    va = [c for c in cases if c["path"] == "valu"]
    assert {c["L"] for c in mf} >= set(C.LENGTHS) and max(c["L"] for c in cases) == 577
    big = [c for c in mf if c["L"] == 577]
    assert all(c["B"] * c["A"] <= 6 for c in big) and any((c["B"], c["A"]) == (2, 3) for c in big)
    assert {c["A"] for c in mf} == {1, 2, 3} and {c["B"] for c in mf} >= {1, 2, 3, 5}
    assert {c["B"] * c["A"] for c in mf if c["order"] == 1} >= {9, 15, 8, 6}
    assert {(c["enc"], c["dh"]) for c in va} == {(e, d) for e in (C.F32, C.BF16, C.F16) for d in C.VALU_DH}
    assert all(c["L"] <= 129 and c["dh"] <= C.VALU_MAX_DH for c in va) and all(c["dh"] == C.MFMA_DH for c in mf)
    for enc in (C.BF16, C.F16):
        sub = [c for c in mf if c["enc"] == enc]
        assert {c["vals"] for c in sub} == set(C.VALUE_SETS) and {c["dscale"] for c in sub} == set(C.DSCALES)
        assert {c["p"] for c in sub} == {0.0, 0.1} and any(c["zero_dctx"] for c in sub)
        for plan in ("lens", "qlim"):
            assert {c["p"] for c in sub if c.get(plan)} == {0.0, 0.1}, (enc, plan)
    assert any(c["ctx2"] for c in mf) and all(c["enc"] == C.F16 for c in mf if c["ctx2"])
    assert {c["planes"] for c in mf} == set(C.PLANES) and {c["order"] for c in mf} == {0, 1}
    assert {c["mask"]["kind"] for c in mf} == set(C.DENSE_KINDS) | {"family"}
    fams = [f for c in mf if c["mask"]["kind"] == "family" for f in c["mask"]["fam"]]
    assert set(fams) == set(C.FAMILY_ID)
    assert any(len(set(c["mask"]["fam"])) > 1 for c in mf if c["mask"]["kind"] == "family")            # mixed batches
    assert {c["mask"]["via"] for c in mf if c["mask"]["kind"] == "family"} == {"build", "pack"}
    q = [v for c in mf if c.get("qlim") for v in c["qlim"]]
    assert set(q) >= {0, 1, 32, 33, 64, 128}
    assert any(v == lv for c in mf if c.get("qlim") for v, lv in zip(c["qlim"], C.row_plan(c)[0]))
    lens = [v for c in mf if c.get("lens") for v in c["lens"]]
    assert set(lens) >= {1, 33, 64, 65} and any(v == c["L"] for c in mf if c.get("lens") for v in c["lens"])
    for c in mf:
        if c.get("lens") and c["mask"]["kind"] == "family":
            assert set(c["mask"]["fam"]) <= set(C.PACKABLE), c
        if c.get("qlim"):
            assert set(c["mask"]["fam"]) <= {"full", "s2s"}, c
    # descriptors at 1, a 32 boundary, a 64 boundary, one past it, and L
    n = [v for c in mf if c["mask"]["kind"] == "family" for v in c["mask"]["n2"] + c["mask"]["vl"]]
    assert {1, 32, 33, 64, 65} <= set(n) and any(v == c["L"] for c in mf if c["mask"]["kind"] == "family" for v in c["mask"]["vl"])


def test_generated_cases_are_inside_the_abi():
    for c in C.all_cases():
        Lv, Lq, cu = C.row_plan(c)
        assert 0 < c["L"] and (c["L"] + 63) // 64 <= C.MAX_T and 0 < c["dh"] <= C.VALU_MAX_DH, c
        assert all(1 <= v <= c["L"] for v in Lv) and all(0 <= v for v in Lq), c
        if c["path"] == "valu":
            assert not c.get("lens") and not c.get("qlim") and not c["ctx2"], c
        how, arg = C.mask_argument(c)
        assert (how == "build") == (c["mask"]["kind"] == "family" and c["mask"]["via"] == "build"), c
        if c["mask"]["kind"] == "family":
            for f, n2, vl in zip(c["mask"]["fam"], c["mask"]["n2"], c["mask"]["vl"]):
                assert 1 <= n2 <= c["L"] and 1 <= vl <= c["L"], c


def test_constants_match_the_sources():
    src = C.attn_source()
    for name, val in (("FWD_NS", C.FWD_NS), ("DQ_NS", C.DQ_NS), ("DKV_NS", C.DKV_NS)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == val
    assert float(re.search(r"#define MASK_ADD \((-?[\d.]+)f\)", src).group(1)) == C.MASK_ADD
    assert len(re.findall(r"if \(T > (\d+)\) return MV_E_SHAPE;", src)) == 2
    assert {int(t) for t in re.findall(r"if \(T > (\d+)\) return MV_E_SHAPE;", src)} == {C.MAX_T}
    assert {int(t) for t in re.findall(r"if \(dh != (\d+)\) return MV_E_SHAPE;", src)} == {C.MFMA_DH}
    assert {int(t) for t in re.findall(r"if \(dh > (\d+) \|\| cu \|\| qlim\) return MV_E_SHAPE;", src)} == {C.VALU_MAX_DH}
    assert re.search(r"att_wait_vmcnt<3 \* PPW>", src) and max(C.FWD_NS, C.DQ_NS, C.DKV_NS) - 1 == 3      # the deepest counted wait
    hdr = open(HDR).read()
    m = re.search(r"dh must be (\d+) \(bf16 MFMA path\) or <= (\d+) \(f32 path\)", hdr)          # the dh limits as the header states them
    assert (int(m.group(1)), int(m.group(2))) == (C.MFMA_DH, C.VALU_MAX_DH)
    assert re.search(r"0 full, 1 s2s, 2 BAR, 3 non-cross, 4 1-D", src)
    assert C.FAMILY_ID == {"full": 0, "s2s": 1, "bar": 2, "noncross": 3, "1d": 4}
    assert C.drop_thr(0.1, 16) == 6554 and C.drop_thr(0.1, 12) == 410 and C.drop_thr(0.1, 8) == 26       # the figures the source comments state


def test_mask_restatement_equals_the_data_module():
    from medvill_amd import data as D
    for fam in C.FAMILY_ID:
        for N, S, n_ids in ((5, 29, [3, 30, 17]), (30, 98, [2, 99, 35]), (62, 64, [1, 2, 65])):
            L, n2 = N + S + 3, N + 2
            m = D.build_mask(fam, N, S, torch.tensor(n_ids))
            m = m if m.dim() == 3 else m[:, None, :].expand(-1, L, -1)
            cfg = dict(seed=0, B=len(n_ids), L=L, mask=dict(kind="family", fam=[fam] * len(n_ids), n2=[n2] * len(n_ids), vl=[n2 + n for n in n_ids]))
            assert torch.equal(C.dense_mask(cfg), m.bool()), (fam, N, S)


def test_tile_classes_and_bits_on_hand_made_masks():
    L = 130
    d = torch.ones((1, L, L), dtype=torch.bool)
    assert C.tile_classes(d).tolist() == [[[1, 1, 1]] * 3]                    # ragged tiles count their existing columns and rows
    d[0, :64, 64:128] = False
    assert C.tile_classes(d)[0, 0].tolist() == [1, 0, 1]
    d[0, 5, :] = False                                                         # a dead row: rows_ok fails, nothing of the tile row is class 0
    assert C.tile_classes(d)[0, 0].tolist() == [2, 2, 2] and C.tile_classes(d)[0, 1].tolist() == [1, 1, 1]
    bits = C.pack_bits(d)
    assert bits.shape == (1, L, 5) and int(bits[0, 0, 0]) == -1 and int(bits[0, 0, 2]) == 0 and int(bits[0, 0, 4]) == 3 and int(bits[0, 5].abs().sum()) == 0


def test_block_maps_are_permutations_and_order_1_groups_by_eight():
    for nxb, A, B in ((2, 3, 3), (1, 3, 5), (3, 2, 3), (5, 2, 4), (2, 1, 5), (4, 1, 1)):
        m0, m1 = C.att_block_map(0, nxb, A, B), C.att_block_map(1, nxb, A, B)
        assert sorted(m0) == sorted(m1) == sorted((x, h, b) for x in range(nxb) for h in range(A) for b in range(B))
        assert [x for x, _, _ in m0] == sorted(x for x, _, _ in m0)                        # order 0: the row block is the slowest index
        full = (A * B) // 8 * 8
        for flat, (x, h, b) in enumerate(m1):
            pair = b * A + h
            if flat < full * nxb:
                assert pair % 8 == flat % 8 and pair // 8 == flat // (8 * nxb) and x == (flat // 8) % nxb
            else:
                assert pair >= full and x == (flat - full * nxb) % nxb                      # the remainder walks the row blocks fastest
    assert C.dropmask_block_map(12, 4) == [0, 3, 6, 9, 1, 4, 7, 10, 2, 5, 8, 11] and C.dropmask_block_map(13, 4) == list(range(13))
    assert sorted(C.dropmask_block_map(24, 6)) == list(range(24))


# ---------------------------------------------------------------------------------------------------------------------
# references against independent formulations
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_reference_equals_explicit_loops():
    cfg = dict(seed=3, path="mfma", enc=C.BF16, B=2, L=7, A=2, dh=4, mask=dict(kind="random"), p=0.1, planes=16, lens=[7, 5], vals="unit", dscale=1.0,
               zero_dctx=False)
    qkv, _ = C.inputs(cfg)
    qkv = qkv.double()
    dense, keep, ik = C.dense_mask(cfg), C.cpu_keep(cfg), C.inv_keep(0.1, 16)
    r = C.ref_forward(qkv, dense, 2, [7, 5], keep, ik)
    H = 8
    for b, Lv in enumerate((7, 5)):
        for h in range(2):
            for i in range(Lv):
                s = [sum(float(qkv[b, i, h * 4 + d]) * float(qkv[b, j, H + h * 4 + d]) for d in range(4)) / 2.0 + (0.0 if dense[b, i, j] else -10000.0)
                     for j in range(Lv)]
                mx = max(s)
                z = sum(math.exp(v - mx) for v in s)
                assert abs(float(r["lse"][b, h, i]) - (mx + math.log(z))) < 1e-12
                for d in range(4):
                    o = sum(math.exp(s[j] - mx) / z * (ik if keep[b, h, i, j] else 0.0) * float(qkv[b, j, 2 * H + h * 4 + d]) for j in range(Lv))
                    assert abs(float(r["ctx"][b, i, h * 4 + d]) - o) < 1e-12


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_backward_reference_equals_autograd_of_a_dense_softmax(p):
    cfg = dict(seed=4, path="mfma", enc=C.F16, B=2, L=70, A=2, dh=8, mask=dict(kind="random"), p=p, planes=16, lens=[70, 41], qlim=[33, 70], vals="unit",
               dscale=1.0, zero_dctx=False)
    Lv, Lq, _ = C.row_plan(cfg)
    qkv, dctx = (t.double() for t in C.inputs(cfg))
    dense, keep, ik = C.dense_mask(cfg), C.cpu_keep(cfg), C.inv_keep(p, 16)
    qd = qkv.clone().requires_grad_(True)
    H, L = 16, 70
    q, k, v = (t.view(2, L, 2, 8).permute(0, 2, 1, 3) for t in qd.split(H, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(8) + (~dense)[:, None].double() * -10000.0
    s = s.masked_fill(torch.arange(L).view(1, 1, 1, L) >= torch.tensor(Lv).view(2, 1, 1, 1), -math.inf)
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.double() * ik
    ctx = (pr @ v).permute(0, 2, 1, 3).reshape(2, L, H)
    rows = (torch.arange(L).view(1, L) < torch.tensor(Lq).view(2, 1)).unsqueeze(-1)
    (ctx * dctx * rows).sum().backward()
    f = C.ref_forward(qkv, dense, 2, Lv, keep, ik)
    assert float((f["ctx"] - ctx.detach()).abs().max()) < 1e-12
    r = C.ref_backward(qkv, f["ctx"], dctx, f["lse"], dense, 2, Lv, Lq, keep, ik)
    got = torch.cat([r["dq"], r["dk"], r["dv"]], dim=-1)
    exist = (torch.arange(L).view(1, L) < torch.tensor(Lv).view(2, 1)).unsqueeze(-1)
    assert float(((got - qd.grad) * exist).abs().max()) < 1e-12
    assert float((r["dq"] * ~rows).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the stand-in against the bounds
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_cases():
    """every 16-bit MFMA case of the sweep"""
    return C.mfma_cases() + C.dense_cases() + C.knob_cases()


def _run_standin(cfg, bug=None):
    """ratios error / bound of the stand-in on one case: dict(ctx, lse, delta, dq, dk, dv).  One sample at a time: the [A, L, L] fp64
    intermediates of the bounds stay small at L = 577."""
    enc, A, B, L = cfg["enc"], cfg["A"], cfg["B"], cfg["L"]
    Lv_, Lq_, _ = C.row_plan(cfg)
    qkv_, dctx_ = C.inputs(cfg)
    dense_, keep_, ik = C.dense_mask(cfg), C.cpu_keep(cfg), C.inv_keep(cfg["p"], cfg["planes"])
    out = dict(ctx=0.0, lse=0.0, dq=0.0, dk=0.0, dv=0.0, delta=0.0)
    for b in range(B):
        qkv, dctx, dense, keep, Lv, Lq = qkv_[b:b + 1], dctx_[b:b + 1], dense_[b:b + 1], None if keep_ is None else keep_[b:b + 1], Lv_[b:b + 1], Lq_[b:b + 1]
        f = C.ref_forward(qkv.double(), dense, A, Lv, keep, ik)
        b_ctx, b_lse = C.fwd_bounds(f, enc, Lv, ik)
        ctx, lse = C.standin_forward(qkv, dense, A, Lv, Lq, enc, keep, ik, bug)
        qrow = torch.arange(L).view(1, L) < torch.tensor(Lq).view(1, 1)
        got = dict(ctx=C.worst_ratio(ctx, f["ctx"], b_ctx, qrow.unsqueeze(-1))[0], lse=C.worst_ratio(lse, f["lse"], b_lse, qrow.unsqueeze(1))[0])
        ctx_in, lse_in = f["ctx"].to(C.DT[enc]), f["lse"].float()
        r = C.ref_backward(qkv.double(), ctx_in.double(), dctx.double(), lse_in.double(), dense, A, Lv, Lq, keep, ik)
        bb = C.bwd_bounds(r, enc, Lv, ik)
        dq, dk, dv, delta = C.standin_backward(qkv, ctx_in, dctx, lse_in, dense, A, Lv, Lq, enc, keep, ik, bug)
        exist = (torch.arange(L).view(1, L) < torch.tensor(Lv).view(1, 1)).unsqueeze(-1)
        for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            got[name] = C.worst_ratio(g, r[name], bb[name], exist)[0]
        got["delta"] = C.worst_ratio(delta, r["delta"], bb["delta"], qrow.unsqueeze(1))[0]
        out = {k: max(out[k], got[k]) for k in out}
    return out


@pytest.fixture(scope="module")
def standin_ratios():
    return [(c, _run_standin(c)) for c in _cpu_cases()]


def test_the_stand_in_stays_below_half_of_every_bound(standin_ratios):
    worst = {}
    for c, r in standin_ratios:
        for name, v in r.items():
            key = (name, c["enc"])
            if v > worst.get(key, (0.0, None))[0]:
                worst[key] = (v, C.case_id(c))
    for key in sorted(worst):
        print(f"    stand-in {key[0]:6s} {key[1]:5s} worst error / bound {worst[key][0]:.3f}   ({worst[key][1]})")
    assert len(standin_ratios) == len(C.mfma_cases()) + len(C.dense_cases()) + len(C.knob_cases())
    assert all(v[0] <= 0.5 for v in worst.values()), worst


@pytest.mark.parametrize("bug", C.BUGS)
def test_a_wrong_stand_in_breaks_a_bound(bug):
    outputs = {"no_alpha": ("ctx", "lse"), "tail_off_by_one": ("ctx", "lse"), "mask_word_off_by_one": ("ctx", "lse"), "no_inv_keep": ("ctx", "dq", "dk", "dv"),
               "delta_not_subtracted": ("dq", "dk"), "dk_dv_swapped": ("dk", "dv")}[bug]
    hits = 0
    for c in _cpu_cases():
        r = _run_standin(c, bug)
        hits += any(r[o] > 1.0 for o in outputs)
        if hits >= 3:
            break
    assert hits >= 3, (bug, hits)


def test_the_gpu_file_iterates_every_generator():
    tree = ast.parse(open(GPU_FILE).read())
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
              and isinstance(n.func.value, ast.Name) and n.func.value.id == "C"}
    assert {"mfma_cases", "dense_cases", "knob_cases", "valu_cases", "mask_cases"} <= called, called
    marks = [d for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) for d in n.decorator_list]
    src = open(GPU_FILE).read()
    assert "skip" not in src and "xfail" not in src and len(marks) >= 4
