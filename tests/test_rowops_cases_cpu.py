"""Branch census of the row-kernel sweep (CPU).  tests/test_rowops_fuzz_gpu.py is only worth its GPU time while its cases reach the
launcher branches of csrc/mv_rowops.hip that the fixed-shape tests never take; this file counts them, checks the caps the
predicates rely on against the .hip source, checks that no case can be dropped, and checks every fp64 reference once against an
independent formulation."""
import os
import re

import numpy as np
import pytest
import torch

import rowops_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc", "mv_rowops.hip")
GPU_FILE = os.path.join(ROOT, "tests", "test_rowops_fuzz_gpu.py")
MIN_HITS = 3

# every launcher branch the sweep exists for, by family (names as the predicates of rowops_cases.py give them)
REQUIRED = {
    "ce": ["scalar8", "scalar128", "vec", "vec_rowwalk", "scalar128:ld%4", "scalar128:ldd%4", "scalar128:logits_misaligned",
           "scalar128:dlogits_misaligned", "scalar128:ldd>32768", "logits_f32", "logits_bf16", "logits_f16", "dlogits_f32", "dlogits_bf16",
           "dlogits_f16", "dlogits_absent", "ties_same_vector+other_wave+last_column", "label_in_padded_last_vector", "labels_mixed",
           "labels_all_ignored", "labels_oob", "scale_dev", "scale_host", "scale_host_x_loss"],
    "ln": ["fwd_nc1", "fwd_nc3", "fwd_nc4", "fwd_nc8", "fwd_ragged_last_chunk", "fwd_y_bf16", "M=1", "fwd_M%4"]
          + [f"fwd_{y}_from_{x}" for y, x in C.LN_FWD_PAIRS] + [f"bwd_{d}_x_{x}" for d, x in C.LN_BWD_PAIRS]
          + ["bwd_pf8", "bwd_plain", "bwd_pf4", "bwd_pf16", "bwd_wide_refused", "bwd_row_walk", "bwd_M%wpb", "bwd_ragged_last_chunk",
             "bwd_dropout", "bwd_no_dropout", "bwd_nc1", "bwd_nc3", "bwd_nc4", "bwd_nc8"],
    "gs": [f"{op}_{dt}" for op in ("gather", "scatter", "scatter_acc") for dt in (C.F32, C.BF16, C.F16)]
          + ["one_pass", "column_loop", "H>768", "ragged_last_pass", "lds!=H!=ldd", "negative_rows", "R%4"],
    "cs": ["colsum_f32", "colsum_bf16", "colsum_f16", "vector_only", "vector+scalar_tail", "scalar_tail_only", "scalar_ldx",
           "scalar_misaligned_base", "one_row_slice", "row_slices>1", "ysplit_capped", "accumulate", "overwrite", "unscale", "no_unscale"],
    "cp": ["partials_one_slice", "partials_row_slices>1", "P<8", "P%4", "N%64", "ld>N", "unscale", "no_unscale"],
    "ew": [f"cast_{s}_to_{d}" for s, d in C.CAST_PAIRS] + ["cast_tail_only", "cast_vector+tail", "cast_vector_only", "cast_grid_stride"]
          + [f"cast2d_{s}_to_{d}" for s, d in C.CAST2D_PAIRS] + ["cast2d_second_launch", "cast2d_column_stride", "cast2d_zero_fill"]
          + [f"add_{dt}" for dt in (C.F32, C.BF16, C.F16)] + [f"dact{m}_{dt}" for m in (0, 1, 2) for dt in (C.F32, C.BF16, C.F16)]
          + ["add_grid_stride", "dact_grid_stride", "transpose_f32", "transpose_bf16", "transpose_f16"],
    "nf": ["count_clean", "count_planted", "count_tail_only", "count_only_in_tail", "count_in_tail", "count_grid_stride", "count_start=0",
           "count_start=5"],
    "aw": ["adamw_tail_only", "adamw_vector+tail", "adamw_vector_only", "adamw_tail_both_shadows", "adamw_grid_stride", "adamw_shadows_both",
           "adamw_shadows_bf16", "adamw_shadows_f16", "adamw_shadows_none", "adamw_state_none", "adamw_state_live", "adamw_state_skip",
           "adamw_correct_bias=0", "adamw_correct_bias=1", "adamw_grad_scale", "adamw_no_grad_scale"],
    "dm": ["mask_p=0", "mask_p=0.1", "mask_p=0.5", "mask_odd_n", "mask_even_n", "mask_grid_stride", "mask_statistics"],
}


@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_every_named_branch_is_reached(fam):
    count = C.census(fam)
    print(f"\n{fam}: {len(C.FAMILIES[fam][0]())} cases")
    for name in sorted(set(REQUIRED[fam]) | set(count)):
        print(f"    {name:48s} {count.get(name, 0):4d}{'' if name in REQUIRED[fam] else '   (not required)'}")
    short = {n: count.get(n, 0) for n in REQUIRED[fam] if count.get(n, 0) < MIN_HITS}
    assert not short, f"{fam}: branches reached fewer than {MIN_HITS} times: {short}"


def test_the_issue_value_sets_are_all_drawn():
    """every shape value the sweep is specified over occurs in at least one case"""
    def seen(fam, key):
        return {c[key] for c in C.FAMILIES[fam][0]() if key in c}
    assert seen("ce", "V") == set(C.CE_V) and seen("ce", "R") == set(C.CE_R)
    assert {C.CE_LDD_WIDE} <= seen("ce", "ldd")
    assert seen("ln", "H") == set(C.LN_H) and seen("ln", "M") == set(C.LN_M) and seen("ln", "variant") == {0, 1, 2, 3}
    assert seen("gs", "H") == set(C.GS_H) and seen("gs", "R") == set(C.GS_R)
    assert seen("cs", "N") == set(C.CS_N) and seen("cs", "M") == set(C.CS_M)
    assert seen("cp", "P") == set(C.CP_P) and seen("cp", "N") == set(C.CP_N)
    assert set(C.CAST_N) | {C.CAST_BIG_N} <= seen("ew", "n")
    assert seen("ew", "rows") >= {1, 64, C.CAST2D_BIG_ROWS}
    assert seen("nf", "n") == set(C.NF_N) | {C.NF_BIG_N}
    assert seen("aw", "n") >= set(C.AW_N) | {C.AW_BIG_N}
    assert seen("dm", "n") == set(C.DM_N) and seen("dm", "p") == set(C.DM_P)
    # at least a third of the cross-entropy cases force ties, and some case ignores every label
    ce = C.ce_cases()
    assert 3 * sum(c["ties"] for c in ce) >= len(ce)


def test_generated_cases_are_inside_the_abi():
    """A generator that draws what the launcher rejects is a bug in the generator: the GPU file has no way to drop a case."""
    for c in C.ce_cases():
        assert c["ld"] >= c["V"] and c["V"] <= C.CE_MAX_V and (c["ddt"] is None or c["ldd"] >= c["V"]), c
        assert (c["ldt"], c["ddt"]) in C.CE_PAIRS, c
    for c in C.ln_cases():
        assert c["H"] % 4 == 0 and 0 < c["H"] <= C.LN_MAX_H and c["M"] > 0, c
        assert (c["ydt"], c["xdt"]) in C.LN_FWD_PAIRS and (c["ddt"], c["xdt"]) in C.LN_BWD_PAIRS, c
        assert not c["y_bf16"] or c["ydt"] == C.F16, c
    for c in C.gs_cases():
        assert c["H"] % 4 == 0 and c["lds"] % 4 == 0 and c["ldd"] % 4 == 0 and c["lds"] >= c["H"] and c["ldd"] >= c["H"], c
        rows = C.gs_rows(c)
        pos = rows[rows >= 0]
        assert len(set(pos.tolist())) == len(pos) and (pos < c["n_other"]).all() and int((rows < 0).sum()) == c["n_neg"], c
    for c in C.cs_cases():
        assert c["ldx"] >= c["N"], c
    for c in C.cp_cases():
        assert c["ld"] >= c["N"], c
    for c in C.ew_cases():
        if c["op"] == "cast":
            assert (c["src"], c["dst"]) in C.CAST_PAIRS
        elif c["op"] == "cast2d":
            assert (c["src"], c["dst"]) in C.CAST2D_PAIRS and c["lds"] >= c["cols"] and c["ldd"] >= c["cols"], c
            assert c["rows"] <= C.CAST2D_ROWS_PER_LAUNCH or c["ldd"] < c["lds"], c
        elif c["op"] in ("add", "dact"):
            assert c["n"] % 4 == 0, c


def test_the_gpu_file_cannot_drop_a_case():
    import ast
    src = open(GPU_FILE).read()
    tree = ast.parse(src)
    for node in ast.walk(tree):
        assert not isinstance(node, (ast.Continue, ast.Break)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):                      # pytest.skip / pytest.xfail / pytest.importorskip / pytest.mark.skip(if) / .xfail
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            assert "unittest" not in ast.dump(node), f"line {node.lineno}"
    # one parametrised test per family, each over the full case list of rowops_cases.py
    for fam, (cases, _) in C.FAMILIES.items():
        assert re.search(r'parametrize\("cfg", C\.%s\(\)' % cases.__name__, src), cases.__name__


def _body(src, name):
    """text of the launcher `extern "C" int name(...) {...}` up to the next top-level definition"""
    i = src.index('extern "C" int %s(' % name)
    j = src.find("\n}\n", i)
    return src[i:j]


def test_the_caps_in_the_source_are_the_caps_of_the_predicates():
    src = open(HIP).read()

    def num(body, pattern):
        m = re.search(pattern, body)
        assert m, pattern
        return int(m.group(1))
    ce = _body(src, "mv_ce_fwd_bwd")
    assert num(ce, r"V > (\d+) &&") == C.CE_SCALAR8_MAX_V
    assert num(ce, r"ldd <= 1024 \* (\d+)") * 1024 == C.CE_VEC_MAX and num(ce, r"V <= 1024 \* (\d+)") * 1024 == C.CE_VEC_MAX
    assert num(ce, r"vgrid\(R < (\d+) \? R : \1\)") == C.CE_VEC_ROWS
    assert num(ce, r"if \(V <= 256 \* (\d+)\) hipLaunchKernelGGL\(\(ce_kernel<TL, TD, 8>") * 256 == C.CE_SCALAR8_MAX_V
    assert num(src, r"#define CE_MAXPER (\d+)") * 256 == C.CE_MAX_V
    assert "ce_vec_kernel<TL, TD, 8, 1024>" in ce                 # 8 vectors x 1024 threads x 4 columns = CE_VEC_MAX
    assert num(src, r"#define MV_MAX_H (\d+)") == C.LN_MAX_H
    disp = open(os.path.join(os.path.dirname(HIP), "mv_dispatch.h")).read()       # the row kernels' chunk count: mv_with_row_chunks
    m = re.search(r"mv_with_row_chunks\(int H,.*?H <= (\d+)\) return f\(std::integral_constant<int, 1>.*?H <= (\d+)\) return f\(std::integral_constant<int, 3>"
                  r".*?H <= (\d+)\) return f\(std::integral_constant<int, 4>.*?return f\(std::integral_constant<int, 8>", disp, re.S)
    assert m and tuple(int(x) for x in m.groups()) == C.LN_NC_STEPS
    lnb = _body(src, "mv_layernorm_bwd")
    m = re.search(r"var == 0 \? (\d+) : var == 3 \? (\d+) : (\d+)\);", lnb)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (C.LN_BWD_CAPS[0], C.LN_BWD_CAPS[3], C.LN_BWD_CAPS[2])
    assert C.LN_BWD_CAPS[1] == C.LN_BWD_CAPS[2]
    m = re.search(r"wpb = var == 0 \? (\d+) : var == 3 \? (\d+) : (\d+);", lnb)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (C.LN_BWD_WPB[0], C.LN_BWD_WPB[3], C.LN_BWD_WPB[2])
    assert num(lnb, r"!\(H <= (\d+) && x_dtype != MV_F32\)\) var = 2;") == C.LN_WIDE_MAX_H
    assert num(_body(src, "mv_layernorm_fwd"), r"grid\(\(M \+ 3\) / (\d+)\)") == 4
    cs = _body(src, "mv_colsum")
    assert num(cs, r"want = \((\d+) \+ xb - 1\) / xb") == C.COLSUM_BLOCKS
    assert re.search(r"strip = \(dtype == MV_F32\) \? 128 : 256;", cs) and re.search(r"ysplit = \(M \+ 255\) / 256;", cs)
    cp = _body(src, "mv_colsum_partials")
    assert num(cp, r"ys = \((\d+) \+ xb - 1\) / xb") == C.PARTIALS_BLOCKS and re.search(r"ys > \(P \+ 7\) / 8", cp)
    for name in ("mv_add", "mv_dact", "mv_cast", "mv_count_nonfinite"):
        assert num(_body(src, name), r"if \(blocks > (\d+)\) blocks = \1;") == C.ELEMWISE_BLOCKS, name
    assert num(_body(src, "mv_adamw_step"), r"if \(blocks > (\d+)\) blocks = \1;") == C.ADAMW_BLOCKS
    assert num(_body(src, "mv_dropout_mask"), r"if \(blocks > (\d+)\) blocks = \1;") == C.DROPMASK_BLOCKS
    c2 = _body(src, "mv_cast2d")
    assert num(c2, r"r0 \+= (\d+)\)") == C.CAST2D_ROWS_PER_LAUNCH and num(c2, r"if \(bx > (\d+)\) bx = \1;") == C.CAST2D_COL_BLOCKS
    # sizes derived from the caps
    assert C.CAST_BIG_N // 4 > C.ELEMWISE_BLOCKS * 256 and C.CAST_BIG_N % 4 == 3
    assert C.AW_BIG_N // 4 > C.ADAMW_BLOCKS * 256 and C.AW_BIG_N % 4 == 1
    assert C.CAST2D_BIG_ROWS > C.CAST2D_ROWS_PER_LAUNCH and C.CAST2D_WIDE_LDD > C.CAST2D_COL_BLOCKS * 256


# ---- the references against independent formulations (fp64 against fp64: 1e-12 relative) --------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def test_cross_entropy_reference_equals_log_softmax_by_hand():
    cfg = dict(C.ce_case(4), R=37, V=1000, ld=1000, ldd=1000, ties=True, labels="oob")
    x, lab, tie_rows = C.ce_inputs(cfg)
    assert tie_rows and {m for m, _ in tie_rows.values()} == {"same_vec", "other_wave", "last"}
    x64 = x.double()
    nll, cnt, hits, grad = C.ce_reference(x64, lab, 0.125)
    nll2, grad2 = C.ce_reference_by_hand(x64, lab)
    assert abs(nll - nll2) <= 1e-12 * abs(nll2) and _rel(grad, 0.125 * grad2) < 1e-12
    valid = (lab >= 0) & (lab < 1000)
    assert cnt == int(valid.sum()) and 0 < cnt < 37
    # the first-maximum rule, and that the tied rows tell it from any other rule
    assert torch.equal(C.first_argmax(x64), torch.from_numpy(np.argmax(x64.numpy(), axis=1)))
    last = torch.tensor([int(np.flatnonzero(r == r.max())[-1]) for r in x64.numpy()])
    assert hits == int(((torch.from_numpy(np.argmax(x64.numpy(), axis=1)) == lab) & valid).sum())
    assert hits != int(((last == lab) & valid).sum())
    # a batch without a labelled row: no loss, no gradient
    nll0, cnt0, hits0, grad0 = C.ce_reference(x64, torch.full_like(lab, -100), 1.0)
    assert (nll0, cnt0, hits0) == (0.0, 0, 0) and float(grad0.abs().max()) == 0.0


def test_adamw_reference_equals_the_known_answers(golden_dir):
    z = np.load(os.path.join(golden_dir, "adamw.npz"))
    lr, b1, b2, eps, wd = [float(x) for x in z["hyper"]]
    from oracle.cxrbert_oracle import hf_adamw_step
    p = torch.tensor(z["p0"], dtype=torch.float64)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t in range(1, 4):
        hf_adamw_step(p, torch.tensor(z["grads"][t - 1], dtype=torch.float64), m, v, t, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd)
        assert _rel(p, torch.tensor(z["p"][t - 1], dtype=torch.float64)) < 1e-12
    assert _rel(m, torch.tensor(z["m"])) < 1e-12 and _rel(v, torch.tensor(z["v"])) < 1e-12
    # the wrapper the GPU test uses: same steps with f32-rounded hyper-parameters, so only 1e-7-close to the golden values
    grads = [torch.tensor(g, dtype=torch.float32) for g in z["grads"]]
    ref = C.hf_adamw_reference(torch.tensor(z["p0"], dtype=torch.float32), grads, lr, b1, b2, eps, wd, 1, 1.0)
    assert len(ref) == 3 and _rel(ref[2][0], torch.tensor(z["p"][2], dtype=torch.float64)) < 1e-6


def test_layernorm_reference_equals_the_closed_form():
    cfg = dict(C.ln_case(7), M=37, H=100)
    x, gamma, beta, dy, const = C.ln_inputs(cfg)
    assert const is not None and float(x[const].float().var()) == 0.0
    x64, g64, b64, dy64 = x.double(), gamma.double(), beta.double(), dy.double()
    keep = torch.ones(37, dtype=torch.bool)
    keep[const] = False                      # with variance 0 the two formulations differ by rounding times 1 / sqrt(eps)
    ref = C.ln_reference(x64[keep], g64, b64, dy64[keep], 1e-12)
    dx, dgamma, dbeta = C.ln_bwd_closed_form(x64[keep], g64, dy64[keep], 1e-12)
    assert _rel(ref["dx"], dx) < 1e-12 and _rel(ref["dgamma"], dgamma) < 1e-12 and _rel(ref["dbeta"], dbeta) < 1e-12
    y = ref["xhat"] * g64 + b64
    assert _rel(ref["y"], y) < 1e-12
    # the constant row: y is beta exactly
    full = C.ln_reference(x64, g64, b64, dy64, 1e-12)
    assert torch.equal(full["y"][const], b64) and abs(float(full["rstd"][const]) - 1e6) < 1e-3


def test_dropout_mask_restatement_has_the_pair_structure():
    key, n = C.DM_KEYS[0], 65537
    m = C.dm_restated(0.1, key, n)
    assert C.dm_threshold(0.1) == 6554 and C.dm_threshold(0.5) == 32768 and C.dm_threshold(0.0) == 0
    q = 1 - 6554 / 65536
    assert abs(m.mean() - q) < 5 * np.sqrt(q * (1 - q) / n)
    assert np.array_equal(m[:1001], C.dm_restated(0.1, key, 1001)) and C.dm_restated(0.0, key, 9).all()
    # p = 0.5 keeps an element iff the top bit of its half-word is set: both halves come from one hash per pair
    h = C.dm_restated(0.5, key, n)
    assert 0.45 < h[0::2].mean() < 0.55 and 0.45 < h[1::2].mean() < 0.55 and (h != C.dm_restated(0.5, C.DM_KEYS[1], n)).mean() > 0.4


def test_cast_inputs_carry_the_special_values():
    sp = C.special_values()
    assert torch.isnan(sp).sum() == 1 and torch.isinf(sp).sum() == 2
    # ties of both encodings in both directions: the two neighbours are equally far
    for enc, t in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        for v, even in ((1 + t, 1.0), (1 + 3 * t, 1 + 4 * t)):
            assert float(torch.tensor(v, dtype=torch.float32).to(enc)) == even
            assert float(torch.tensor(v, dtype=torch.float32)) == v
    assert torch.isinf(torch.tensor(65520.0).to(torch.float16)) and float(torch.tensor(65519.0).to(torch.float16)) == 65504.0
    for n in C.CAST_N:
        for seed in (0, 5):
            x = C.cast_input(n, C.F32, seed)
            assert x.numel() == n
    x = C.cast_input(1001, C.F32, 3)
    assert torch.isnan(x).sum() == 2 and torch.isinf(x).sum() == 4
