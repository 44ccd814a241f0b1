"""Branch census of the GEMM sweep (CPU).  tests/test_gemm_sweep_gpu.py is only worth its GPU time while its cases reach the routes,
reduce bodies and epilogue paths of csrc/mv_gemm*.hip that the fixed-shape tests never take; this file counts them, checks every
number the predicates rely on against the .hip / .h text, checks that every case is inside the ABI (the GPU file cannot drop one),
shows that a plain f32 computation passes every case's bound while each planted defect fails it, and checks the fp64 references
once against independent formulations."""
import os
import re

import pytest
import torch

import gemm_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc")
GPU_FILE = os.path.join(ROOT, "tests", "test_gemm_sweep_gpu.py")
MIN_HITS = 3


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# every route, reduce body and epilogue path the sweep exists for, by family (names as gemm_cases.plan / conv_branches give them)
_LAYOUTS4 = ["layout_NT", "layout_NN", "layout_TN", "layout_TNN"]
REQUIRED = {
    "small": ["mfma128", "mfma128_2stage", "operands_bf16", "operands_f16", "wide16", "wide16_R", "fast4", "slow", "ragged_last_k_tile",
              "ragged_last_row_tile", "C_f32", "C_bf16", "C_f16", "C3_bf16", "C3_f16", "R_f32", "R_bf16", "R_f16"] + _LAYOUTS4,
    "ring": ["ring14", "pring", "ring320", "ring256x128", "ring_tn4", "variant=14", "variant=24", "variant=10", "variant=2", "variant=4",
             "stages<ring", "stages=ring", "stages>ring", "wide16", "wide16_R", "wide16+ragged_neighbour", "fast4", "fast4_R_ahead", "fast4_R_inline",
             "slow", "csum", "operands_bf16", "operands_f16", "pring_full+ragged_tiles", "pring_ragged_tiles"] + _LAYOUTS4,
    "pring_walk": ["pring", "ring14", "pring_multi_unit_walk", "pring_walk>=3_units_per_block", "pring_epi_ops_wait", "pring_full+ragged_tiles",
                   "accumulate", "epi_BIAS_RES", "slabs=2", "partial_store", "reduce_fast4"] + _LAYOUTS4,
    "valu": ["valu", "operands_bf16", "operands_f16", "operands_f32", "slabs=1", "slabs=2", "slabs=3", "reduce_scalar", "reduce_fast4", "slow",
             "partial_store", "partial_store_ragged", "K%8"] + _LAYOUTS4,
    "auto": ["route_rounds256", "route_rounds320", "route_rounds_back_to_128", "route_wide320", "route_wide256", "pring", "mfma128", "ring14",
             "ring320", "csum", "slabs=4", "slabs=8", "slabs=2"],
    "reduce": [b + s for b in ("reduce_fast4", "reduce_slow4", "reduce_scalar") for s in ("", "+alpha", "+accumulate")]
              + ["mfma128", "ring14", "pring", "valu", "slabs=2", "slabs=4", "slabs=7", "slabs_clamped", "reduce_none", "partial_store", "partial_store_ragged"],
    "workspace": ["reduce_fast4", "reduce_none", "pring", "mfma128"],
    "epi": ["epi_" + n for n in G.EPI_NAMES] + ["mfma128", "mfma128_2stage", "ring14", "pring", "ring320", "wide16", "wide16_R", "fast4", "fast4_R_ahead",
                                                 "fast4_R_inline", "slow", "dropout", "C_f32", "C_bf16", "C_f16", "R_f32", "R_bf16", "R_f16", "C3_bf16", "C3_f16"],
    "conv": ["conv_interior_tile", "conv_tile_with_padding_taps", "conv_tile_crosses_image", "conv_ragged_last_k_tile", "conv_ragged_last_row_tile",
             "conv_k_tile_straddles_taps", "conv_rows>128", "conv_C=8", "conv_C=16", "conv_C=64", "conv_y_f32", "conv_y_bf16", "conv_R_f32", "conv_R_bf16"]
            + ["conv_epi_" + G.EPI_NAMES[e] for e in G.CONV_EPIS],
}
# single routes of the automatic choice and single workspace sizes: the family holds one or two cases of each by construction
MIN_HITS_OF = {("auto", "csum"): 1, ("auto", "slabs=4"): 1, ("auto", "slabs=8"): 1, ("auto", "slabs=2"): 1}


@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_every_named_branch_is_reached(fam):
    count = G.census(fam)
    print(f"\n{fam}: {len(G.FAMILIES[fam]())} cases")
    for name in sorted(set(REQUIRED[fam]) | set(count)):
        print(f"    {name:48s} {count.get(name, 0):4d}{'' if name in REQUIRED[fam] else '   (not required)'}")
    short = {n: count.get(n, 0) for n in REQUIRED[fam] if count.get(n, 0) < MIN_HITS_OF.get((fam, n), MIN_HITS)}
    assert not short, f"{fam}: branches reached fewer than {MIN_HITS} times: {short}"


def test_the_auto_cases_take_the_routes_the_table_names():
    for c, row in zip(G.auto_cases(), G.AUTO_TABLE):
        pl = G.plan(c, 256)
        assert (pl["rule"], pl["kernel"], pl["slabs"]) == row[7], (c, pl)
    # the two cases with the whole-rounds rule switched off are the first two shapes again
    off = [r for r in G.AUTO_TABLE if r[6] == 0]
    assert {r[:4] for r in off} == {G.AUTO_TABLE[0][:4], G.AUTO_TABLE[1][:4]}
    # an explicit slab count above the ring kernels' own wish is clamped, and the predicate says so
    c = G.base("reduce", 0, ta=1, tb=1, M=200, N=136, K=4100, force=2, nj=14, splitk=7, ws="ample")
    assert G.plan(c)["slabs"] == 4 and "slabs_clamped" in G.plan(c)["branches"]
    assert G.plan(dict(c, force=1))["slabs"] == 7


def test_the_issue_value_sets_are_all_drawn():
    def seen(fam, key):
        return {c[key] for c in G.FAMILIES[fam]()}
    assert seen("small", "M") == set(G.SMALL_M) and seen("small", "N") == set(G.SMALL_N) and seen("small", "K") == set(G.SMALL_K)
    assert seen("small", "nj") == {0, 32}
    assert {(c["dt"], G.LAYOUT_OF[(c["ta"], c["tb"])]) for c in G.small_cases()} == set(G.SMALL_DL)
    ring = G.ring_cases()
    assert {(c["nj"], c["dt"], G.LAYOUT_OF[(c["ta"], c["tb"])]) for c in ring} == set(G.RING_COMBOS) and seen("ring", "nj") == set(G.RING_NJ)
    assert seen("ring", "M") == set(G.RING_M) | set(G.RING_M320) and seen("ring", "N") == set(G.RING_N)
    assert {c["M"] for c in ring if c["nj"] == 10} >= set(G.RING_M320)
    assert {c["K"] for c in ring if c["nj"] in (2, 4)} == set(G.RING_K32) and {c["K"] for c in ring if c["nj"] not in (2, 4)} == set(G.RING_K64)
    # a (variant, encoding, layout) is drawn exactly where the launcher has a branch of its own for it
    for nj in G.RING_NJ:
        for dt in (G.BF16, G.F16):
            for lay in G.LAYOUTS:
                assert G.ring_variant_differs(nj, dt, lay) == ((nj, dt, lay) in G.RING_COMBOS), (nj, dt, lay)
    pw = G.pring_cases()
    assert {(c["M"], c["N"]) for c in pw} == set(G.PRING_SHAPES) and {c["pcus"] for c in pw} == set(G.PRING_CUS) and {c["nj"] for c in pw} == {14, 24}
    assert all(c["launches"] == 2 for c in pw)
    assert seen("valu", "M") == set(G.VALU_MN) and seen("valu", "N") == set(G.VALU_MN) and seen("valu", "K") == set(G.VALU_K)
    assert seen("valu", "splitk") == {1, 3} and seen("valu", "dt") == {G.F32, G.BF16, G.F16}
    assert {(c["ta"], c["tb"]) for c in G.valu_cases()} == set(G.LAYOUTS.values())
    rd = G.reduce_cases()
    assert seen("reduce", "splitk") == set(G.REDUCE_SLABS) and seen("reduce", "N") == {136, 200, 130, 135, 137}
    for kname, _ in G.REDUCE_KERNELS:
        for N, pad, off, body in G.REDUCE_SHAPES:
            for acc in (0, 1):
                for al in (None, 0.25):
                    hit = [c for c in rd if G.plan(c)["kernel"] == kname and (c["N"], c["ldc_pad"], c["c_off"], c["accumulate"], c["alpha"]) == (N, pad, off, acc, al)]
                    assert len(hit) == 1 and G.plan(hit[0])["reduce"] in (body, "reduce_none"), (kname, N, pad, off, acc, al)
    assert seen("workspace", "ws") == {"exact", "short", "none"}
    # one float short of the wish: the ring kernels take the slabs that fit, the 128x128 kernel one slab
    for c in G.workspace_cases():
        pl, wish = G.plan(c), G.plan(dict(c, ws="exact"))["slabs"]
        if c["ws"] == "short":
            assert pl["slabs"] == (wish - 1 if pl["kernel"] != "mfma128" else 1), c
        elif c["ws"] == "none":
            assert pl["slabs"] == 1, c
    ep = G.epi_cases()
    assert {(c["M"], c["N"], c["K"]) for c in ep} == set(G.EPI_SHAPES) and seen("epi", "epi") == set(range(11))
    assert {c[k] for c in ep for k in ("ldc_pad", "ldr_pad", "ldc2_pad", "ldc3_pad")} == {0, 8, 4}
    for k in ("c_off", "r_off", "c2_off", "c3_off", "bias_off"):
        assert seen("epi", k) == {0, 1}, k
    assert {c["p_drop"] for c in ep if c["epi"] == G.EPI_BIAS_RES} == {0.0, 0.1}
    cv = G.conv_cases()
    for key, vals in (("C", G.CONV_C), ("O", G.CONV_O), ("k", G.CONV_K), ("s", G.CONV_S), ("p", G.CONV_P), ("B", G.CONV_B)):
        assert {c[key] for c in cv} == set(vals), key
    assert all(5 <= c["H"] <= 13 and 5 <= c["W"] <= 13 and c["H"] != c["W"] for c in cv)
    # a third of the cases carry the 4 x edge chunks
    for fam in G.FAMILIES:
        cs = G.FAMILIES[fam]()
        assert 4 * sum(c["edge4"] for c in cs) >= len(cs), fam


def _abi_error(c):
    """the MV_E_* conditions of mv_gemm restated on a cfg -> None or the name of the first refusal"""
    fl, pl = G.flags(c), G.plan(c)
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    if c["c3dt"] and c["c3dt"] == G.F32:
        return "C3 must be 16-bit"
    if epi in G.NEED_R and c["rdt"] is None:
        return "R"
    sk = c["splitk"] if c["splitk"] >= 0 else 1
    if (sk > 1 or c["accumulate"]) and (epi != G.EPI_NONE or c["cdt"] != G.F32 or c["c3dt"]):
        return "split-K / accumulate: plain f32 C only"
    if sk > 1 and (G.ws_floats(c) is None or G.ws_floats(c) < sk * M * N):
        return "workspace"
    if c["alpha"] is not None and (epi != G.EPI_NONE or c["cdt"] != G.F32 or c["c3dt"]):
        return "alpha"
    if c["p_drop"] > 0 and (epi != G.EPI_BIAS_RES or N % 4):
        return "dropout"
    mfma = c["dt"] != G.F32 and c["impl"] == 0
    if mfma and c["dt"] == G.F16 and c["ta"] and not c["tb"]:
        return "f16 A^T.B^T"
    if c["csum"]:
        if not (mfma and pl["kernel"] == "ring14" and pl["variant"] == 14 and pl["slabs"] == 1 and not c["accumulate"] and fl["vec8_ok"] and N % 256 == 0
                and c["cdt"] != G.F32 and (epi in G.WIDE_E or (epi in (G.EPI_MUL, G.EPI_RES) and fl["r8_ok"]))):
            return "colsum_part"
    if not mfma and G.cdiv(M, 64) > 65535:
        return "grid"
    t = G.gemm_inputs(c)
    if mfma and (t["lda"] % 8 or t["ldb"] % 8):
        return "lda / ldb"
    if t["lda"] < (M if c["ta"] else K) or t["ldb"] < (N if c["tb"] else K):
        return "ld"
    return None


def test_generated_cases_are_inside_the_abi():
    for c in G.all_gemm_cases():
        assert _abi_error(c) is None, (_abi_error(c), c)
        t = G.gemm_inputs(c)
        K8 = G.up(c["K"], 8)
        # the contract on the operands: k-contiguous rows zero-padded to K rounded up to 8, NaN everywhere else outside the logical window
        for name, trans, rows in (("A", c["ta"], c["M"]), ("B", c["tb"], c["N"])):
            st = t[name].float()
            if not trans:
                assert st.shape[0] == rows and bool((st[:, c["K"]:K8] == 0).all()) and bool(torch.isnan(st[:, K8:]).all()), (name, c)
                assert bool(torch.isfinite(st[:, :c["K"]]).all())
            else:
                assert st.shape[0] == c["K"] and bool(torch.isnan(st[:, rows:]).all()) and bool(torch.isfinite(st[:, :rows]).all()), (name, c)
    for c in G.conv_cases():
        Ho, Wo, M, K = G.conv_dims(c)
        assert c["C"] % 8 == 0 and c["C"] & (c["C"] - 1) == 0 and c["O"] % 4 == 0 and Ho > 0 and Wo > 0, c
        assert c["epi"] in G.CONV_EPIS and c["cdt"] in (G.F32, G.BF16) and c["rdt"] in (None, G.F32, G.BF16), c
        assert (c["rdt"] is not None) == (c["epi"] == G.EPI_BIAS_RES_RELU), c
    # some convolution passes 128 rows with an image boundary inside a row tile, and some K-tile straddles filter taps
    assert any({"conv_rows>128", "conv_tile_crosses_image"} <= set(G.conv_branches(c)) for c in G.conv_cases())


def test_the_gpu_file_cannot_drop_a_case():
    import ast
    src = open(GPU_FILE).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
    for fam, gen in G.FAMILIES.items():
        assert re.search(r'parametrize\("cfg", G\.%s\(\)' % gen.__name__, src), gen.__name__


def test_the_constants_in_the_source_are_the_constants_of_the_predicates():
    gemm, common, ring = _src("mv_gemm.hip"), _src("mv_gemm_common.h"), _src("mv_gemm_ring.h")

    def num(text, pattern, group=1):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(group))
    assert (num(gemm, r"#define GT_BM (\d+)"), num(gemm, r"#define GT_BN (\d+)"), num(gemm, r"#define GT_BK (\d+)")) == (G.GT_BM, G.GT_BN, G.GT_BK)
    assert (num(common, r"#define G2_BM (\d+)"), num(common, r"#define G2_BK (\d+)")) == (G.G2_BM, G.G2_BK)
    # the thresholds of the dispatch are named constants of mv_gemm_plan.h; what the plan does with them is compared with plan() call by
    # call in tests/test_gemm_plan_cpu.py
    plan = _src("mv_gemm_plan.h")

    def const(name):
        return num(plan, r"\b%s = (\d+)[,;]" % name)
    assert (const("T128"), const("T128_BK")) == (G.GT_BM, G.GT_BK) and G.GT_BN == G.GT_BM
    assert "static_assert(GT_BM == T128 && GT_BN == T128 && GT_BK == T128_BK" in gemm
    assert (const("RING_ROWS"), const("RING_320_ROWS"), const("RING_BK")) == (G.G2_BM, G.RING_320_ROWS, 2 * G.G2_BK)
    assert (const("VALU_TILE"), const("VALU_BK")) == (G.VALU_TILE, G.VALU_BK)
    for name in ("BIG_MIN_M", "BIG_MIN_N", "BIG_MIN_T128", "BIG_LONG_K", "WIDE_NT_MIN_N", "ROUNDS_MIN_M", "ROUNDS_MIN_N", "ROUNDS_MIN_K", "SLOTS_128", "SLOTS_128_SK",
                 "SLOTS_RING", "SLOTS_RING_V128", "SK_MIN_K", "SK_DEPTH", "SK_CAP_128", "SK_CAP_RING"):
        assert const(name) == getattr(G, name), name
    assert {k: const("ROUND_COST_" + k) for k in G.ROUND_COST} == G.ROUND_COST and {k: const("WIDE_COST_" + k) for k in G.WIDE_COST} == G.WIDE_COST
    assert num(ring, r"constexpr int EPI_OPS = (\d+);") == G.EPI_OPS and ring.count("constexpr int EPI_OPS = %d;" % G.EPI_OPS) == 2
    # the 16-byte-store condition and the epilogue classes it names
    assert ("#define G2_WIDE_COND(NJ_) ((WIDE_E || (WIDE_R && p.r8_ok)) && (NJ_) == 4 && p.vec8_ok && p.c_dtype != MV_F32 && !p.accumulate && "
            "n0 + wn + 64 <= p.N)") in common
    for text in (common, gemm):
        assert "WIDE_E = (E_) == MV_EPI_NONE || (E_) == MV_EPI_BIAS || (E_) == MV_EPI_BIAS_GELU_D;" in text
        assert "WIDE_R = (E_) == MV_EPI_MUL || (E_) == MV_EPI_RES || (E_) == MV_EPI_BIAS_RES;" in text
    assert "if (!CONV && G2_WIDE_COND(NJ))" in gemm and "fast[j] = p.vec_ok && (p.N - n >= 4);" in gemm
    assert "const bool lane_fast = ((E_) >= 0) && col_on && p.vec_ok && (p.N - ncol >= 4);" in common and "if (HAS_R && __all(lane_fast || !col_on))" in common
    assert "const bool full = (m0 + G2_BM <= p.M) && (n0 + BN <= p.N) && ((p.N & 3) == 0) && (p.splitk > 1 || p.vec_ok);" in ring
    # (the launchers' variant tables -- ring_kernel -- are mv_plan_ring_kernel of mv_gemm_plan.h now: tests/test_gemm_plan_cpu.py)
    for k, (bm, bn, bk) in G.RING_TILE.items():
        assert bm in (G.G2_BM, G.RING_320_ROWS) and bn in (256, 128) and bk in (G.G2_BK, 2 * G.G2_BK), k
    # all three bodies of the split-K reduce apply alpha
    red = gemm[gemm.index("__global__ void splitk_reduce_kernel"):gemm.index("// test / experiment hooks")]
    assert red.count("if (p.alpha) s *= *p.alpha;") == 2 and "epilogue4_slow(p, m, n, s);" in red
    assert "const float al = p.alpha ? *p.alpha : 1.0f;" in common
    # the dropout threshold and the tolerances derived from a measurement
    assert G.TANH_TOL == 4 * G.TANH_MEASURED and G.GELU_TOL == 4 * G.GELU_MEASURED
    hdr = open(os.path.join(ROOT, "include", "medvill.h")).read()
    for i, n in enumerate(G.EPI_NAMES):
        assert re.search(r"MV_EPI_%s = %d\b" % (n, i), hdr), n


# ---- the bounds let an honest f32 computation through and catch every planted defect ------------------------------------------------
def _cpu_shape(c):
    """the auto family's large shapes are run on the device only: here one small shape with the same epilogue and outputs"""
    if c["fam"] == "auto" and c["M"] > 3000:
        return dict(c, M=300, N=256 if c["csum"] else 384, K=72, force=2 if c["csum"] else 0, nj=14 if c["csum"] else 0)
    return c


_CACHE = {}


def _evaluated(c):
    """(plan, inputs, references) of a case, computed once for the honest and the defect checks"""
    key = (c["fam"], c["seed"])
    if key not in _CACHE:
        if c["fam"] == "conv":
            t = G.conv_inputs(c)
            _CACHE[key] = (None, t, G.conv_reference(c, t))
        else:
            pl, t = G.plan(c), G.gemm_inputs(c)
            _CACHE[key] = (pl, t, G.gemm_reference(c, t, pl))
    return _CACHE[key]


def _all_cases():
    return [_cpu_shape(c) for c in G.all_gemm_cases()] + G.conv_cases()


def _worst(c, defect=None):
    pl, t, ref = _evaluated(c)
    got = G.honest_conv(c, t, defect) if c["fam"] == "conv" else G.honest_gemm(c, t, pl, defect)
    worst = 0.0
    for name, val in got.items():
        ok, w = G.within(val, *ref[name])
        worst = max(worst, w if ok or w > 1 else float("inf"))
    return worst


def test_an_honest_f32_computation_passes_every_bound():
    worst, at = 0.0, None
    for c in _all_cases():
        w = _worst(c)
        if w > worst:
            worst, at = w, c
        assert w <= 1.0, (w, c)
    print(f"\nhonest f32 computation: worst error / bound = {worst:.3f} at {at['fam']} seed {at['seed']}")
    assert worst > 0.02, "bounds this loose could not see a defect"


@pytest.mark.parametrize("defect", G.DEFECTS)
def test_every_planted_defect_fails_the_bound_of_every_case_it_applies_to(defect):
    cases = [c for c in _all_cases() if G.defect_applies(defect, c)]
    assert len(cases) >= 10, (defect, len(cases))
    passed = [(c["fam"], c["seed"]) for c in cases if _worst(c, defect) <= 1.0]
    weakest = min(_worst(c, defect) for c in cases)
    print(f"\n{defect}: {len(cases)} cases, smallest error / bound under the defect = {weakest:.1f}")
    assert not passed, f"{defect}: not caught in {passed}"


# ---- the references against independent formulations ------------------------------------------------------------------------------
def test_conv_reference_equals_explicit_loops_over_the_taps():
    for c in (G.conv_case(1), G.conv_case(14)):
        t = G.conv_inputs(c)
        Ho, Wo, M, K = G.conv_dims(c)
        ref = G.conv_reference(dict(c, epi=G.EPI_NONE, cdt=G.F32), t)["C"][0]
        loops = G.conv_by_loops(c, t)
        assert float((ref - loops).abs().max()) <= 1e-12 * float(loops.abs().max())
        # and the patch matrix of the honest computation is the same convolution
        pm = G.conv_patches(c, t).double() @ t["w"].double().reshape(c["O"], K).t()
        assert float((pm - loops).abs().max()) <= 1e-12 * float(loops.abs().max())


def test_product_reference_equals_loops_over_the_stored_operands():
    """the reference works on the logical operands; here the product is rebuilt element by element from the STORAGE the kernel is given
    (leading dimensions, transposed layouts, padding), for one case of every layout"""
    for lay, (ta, tb) in G.LAYOUTS.items():
        c = G.base("small", 3, ta=ta, tb=tb, M=5, N=6, K=11, a_pad=8, b_pad=8, force=1)
        t = G.gemm_inputs(c)
        A, B = t["A"].double(), t["B"].double()
        y = torch.zeros((5, 6), dtype=torch.float64)
        for m in range(5):
            for n in range(6):
                for k in range(11):
                    y[m, n] += (A[k, m] if ta else A[m, k]) * (B[k, n] if tb else B[n, k])
        ref = G.gemm_reference(c, t, G.plan(c))["C"][0]
        assert float((ref - y).abs().max()) <= 1e-12, lay


def test_epilogue_references_equal_their_definitions():
    z = torch.linspace(-6, 6, 241, dtype=torch.float64)
    assert float((G.gelu64(z) - torch.nn.functional.gelu(z)).abs().max()) < 1e-14
    zz = z.clone().requires_grad_(True)
    torch.nn.functional.gelu(zz).sum().backward()
    assert float((G.dgelu64(z) - zz.grad).abs().max()) < 1e-14
    assert float(G.dgelu64(z).abs().max()) < G.LIP_GELU
    h = 1e-5
    assert float(((G.dgelu64(z + h) - G.dgelu64(z - h)) / (2 * h)).abs().max()) < G.LIP_DGELU
    # the mask: survivors scaled so that the expectation is kept, pairs share a hash
    keep, inv = G.keep_mask(0.1, 0x1234567800000077, 64, 132)
    assert abs(float(keep.mean()) * inv - 1.0) < 0.02 and set(keep.unique().tolist()) == {0.0, 1.0}
    # column-sum halves: row 2 * tile + half
    c = G.base("ring", 0, M=300, N=256, K=8, force=2, nj=14, cdt=G.BF16, csum=True)
    t = G.gemm_inputs(c)
    ref = G.gemm_reference(c, t, G.plan(c))
    full = ref["C"][0]
    assert ref["csum"][0].shape == (4, 256)
    assert torch.allclose(ref["csum"][0][1], full[128:256].sum(0)) and torch.allclose(ref["csum"][0][2], full[256:300].sum(0))
    assert float(ref["csum"][0][3].abs().max()) == 0.0 and torch.allclose(ref["colsum"][0], full.sum(0))
