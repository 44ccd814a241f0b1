"""Branch census and bound check of the region-encoder support-kernel sweep (CPU).  tests/test_convops_sweep_gpu.py is only worth
its GPU time while its cases reach every launcher branch of csrc/mv_conv.hip and its bounds can tell a right kernel from a wrong
one; this file counts the branches, checks the caps the predicates rely on against the .hip source, checks that no case can be
dropped, and runs an honest f32 restatement of every kernel, and the same restatement with one defect planted at a time, through
the very references and bounds the GPU file asserts."""
import ast
import os
import re

import pytest
import torch

import convops_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc", "mv_conv.hip")
GPU_FILE = os.path.join(ROOT, "tests", "test_convops_sweep_gpu.py")
DEFECT_MAX_ELEMS = 1 << 20       # the planted defects are looked for in the cases below this size: one failing case each is the claim

# every launcher branch the sweep exists for, by family (names as the predicates of convops_cases.py give them)
REQUIRED = {
    "nhwc": ["nhwc_bf16", "nhwc_f32", "nhwc_pad_channels", "nhwc_Cp==C", "nhwc_one_trip", "nhwc_second_trip"],
    "im2col": ["bf16/VEC8", "bf16/VEC4", "f32/VEC4", "VEC4:C%8", "VEC4:ldk%8", "VEC4:misaligned", "ldk_partial_last_group", "ldk_whole_groups",
               "ldk_pad_tail", "ldk==kc", "im2col_one_trip", "im2col_second_trip", "ksp=7/2/3", "ksp=3/1/1", "ksp=3/2/1", "ksp=1/2/0",
               "image_smaller_than_kernel", "kh!=kw"],
    "pool": ["pool_bf16", "pool_f32", "pool_one_trip", "pool_second_trip", "pool_H_odd", "pool_H_even", "pool_W_odd", "pool_W_even",
             "pool_one_pixel_wide"],
    "stats": ["stats_bf16", "stats_f32", "stats_int", "stats_gauss", "stats_gauss_offset", "one_slab", "slabs>1", "slab_cap_binds", "rpb<512",
              "rpb=512", "rpb>512", "walk_ends_pair", "walk_ends_single", "walk_ends_idle", "short_last_slab", "last_column_block_partial",
              "column_blocks_whole", "column_blocks>1", "ldx>C", "ldx==C"],
    "fin": ["fin_running", "fin_no_running", "fin_rows=1", "fin_rows=2", "fin_rows=12544", "fin_running_momentum=0.1", "fin_running_momentum=1",
            "fin_eps=1e-05", "fin_eps=0.001", "fin_one_block", "fin_blocks>1", "fin_partial_last_block", "fin_variance_0_column"],
    "act": ["act_%s_to_%s%sres%srelu" % (x, y, r, l) for x, y in C.ACT_BODIES for r in "+-" for l in "+-"]
           + ["act_%s_to_%s" % b for b in C.ACT_BODIES] + ["act_one_trip", "act_second_trip"],
}


@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_every_named_branch_is_reached(fam):
    count = C.census(fam)
    print(f"\n{fam}: {len(C.FAMILIES[fam][0]())} cases")
    for name in sorted(set(REQUIRED[fam]) | set(count)):
        print(f"    {name:40s} {count.get(name, 0):4d}{'' if name in REQUIRED[fam] else '   (not required)'}")
    missing = [n for n in REQUIRED[fam] if not count.get(n)]
    assert not missing, f"{fam}: branches no case reaches: {missing}"


def test_the_value_sets_of_the_sweep_are_all_drawn():
    def seen(fam, *keys):
        return {tuple(c[k] for k in keys) if len(keys) > 1 else c[keys[0]] for c in C.FAMILIES[fam][0]()}
    assert seen("nhwc", "C", "Cp") == set(C.NHWC_CHANNELS) and {(1, 1)} < seen("nhwc", "H", "W")
    assert {(g[0], g[1], g[2], g[3], g[4], g[5]) for g in C.IM2COL_GEOMS} <= seen("im2col", "kh", "kw", "stride", "pad", "H", "W")
    assert {(C.BF16, 8), (C.BF16, 16), (C.BF16, 3), (C.BF16, 12)} <= seen("im2col", "dt", "C")
    assert {c["ldk"] % 4 for c in C.im2col_cases() if c["dt"] == C.F32} == {0, 1, 3}
    assert any(c["dt"] == C.BF16 and c["C"] == 8 and c["ldk"] % 8 == 4 for c in C.im2col_cases())
    # every geometry meets every dtype / alignment variant
    assert len({(c["kh"], c["kw"], c["stride"], c["H"], c["dt"], c["C"], c["ldk"] - c["kh"] * c["kw"] * c["C"], c["dst_off"])
                for c in C.im2col_cases()}) >= len(C.IM2COL_GEOMS) * len(C.IM2COL_VARIANTS)
    assert set(C.POOL_IMAGES) <= seen("pool", "H", "W") and seen("pool", "C") == set(C.POOL_C)
    assert {(h, w, c, d) for h, w in C.POOL_IMAGES for c in C.POOL_C for d in (C.BF16, C.F32)} <= seen("pool", "H", "W", "C", "dt")
    assert set(C.STATS_ROWS) <= seen("stats", "rows") and seen("stats", "C") == set(C.STATS_C)
    assert {(r, c, "int") for r in C.STATS_ROWS for c in C.STATS_C} <= seen("stats", "rows", "C", "kind")
    for key in ("rows", "C"):                               # each size meets both dtypes and both row pitches
        for v in seen("stats", key):
            cs = [c for c in C.stats_cases() if c[key] == v]
            assert {c["dt"] for c in cs} == {C.BF16, C.F32} or v > 1000, (key, v)
            assert {c["ldx"] > c["C"] for c in cs} == {True, False} or v > 1000, (key, v)
    assert any(C.stats_plan(c["rows"])[1] and c["C"] == 4 for c in C.stats_cases())
    assert seen("fin", "C", "rows", "running") == {(c, r, u) for c in C.FIN_C for r in C.FIN_ROWS for u in (True, False)}
    assert seen("fin", "momentum") == set(C.FIN_MOMENTUM) and seen("fin", "eps") == set(C.FIN_EPS)
    for body in C.ACT_BODIES:
        cs = [c for c in C.act_cases() if (c["xdt"], c["ydt"]) == body]
        assert {c["rows"] for c in cs} >= {1, 3, 1000} and {c["C"] for c in cs} >= {4, 64, 68}, body
    assert set(C.ACT_SHAPES) <= seen("act", "rows", "C")


def test_generated_cases_are_inside_the_abi():
    """A generator that draws what the launcher rejects is a bug in the generator: the GPU file has no way to drop a case."""
    assert C.GUARD % 8 == 0                                  # whole 16-byte vectors in front of every output, in both encodings
    for c in C.nhwc_cases():
        assert c["Cp"] >= c["C"] > 0 and min(c["B"], c["H"], c["W"]) > 0, c
    for c in C.im2col_cases():
        Ho, Wo, rows, kc = C.im2col_shape(c)
        assert Ho > 0 and Wo > 0 and c["ldk"] >= kc and c["pad"] >= 0 and c["stride"] > 0, c
        assert rows * c["ldk"] < 2 ** 31 and c["dst_off"] % 4 == 0, c
    for c in C.pool_cases():
        assert c["C"] % 4 == 0 and min(c["B"], c["H"], c["W"]) > 0, c
    for c in C.stats_cases():
        assert c["C"] % 4 == 0 and c["ldx"] % 4 == 0 and c["ldx"] >= c["C"] and c["rows"] > 0, c
        assert c["kind"] != "int" or 64 * c["rows"] <= 2 ** 24 or (C.stats_int_range(c["rows"]) == 2 and 4 * c["rows"] <= 2 ** 24), c
    for c in C.fin_cases():
        assert c["C"] > 0 and 0 < c["rows"] < 2 ** 24, c
    for c in C.act_cases():
        assert c["C"] % 4 == 0 and c["rows"] > 0 and (c["xdt"], c["ydt"]) in C.ACT_BODIES, c
    # a printed cfg reproduces the case
    for fam, (cases, _) in C.FAMILIES.items():
        seeds = [c["seed"] for c in cases()]
        assert len(set(seeds)) == len(seeds), fam
    a, b = C.stats_inputs(C.stats_case(5)), C.stats_inputs(dict(C.stats_case(5)))
    assert C.same_bits(a, b)


def test_the_gpu_file_cannot_drop_a_case():
    src = open(GPU_FILE).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            assert "unittest" not in ast.dump(node), f"line {node.lineno}"
    for fam, (cases, _) in C.FAMILIES.items():              # one parametrised test per entry point over its full case list
        assert re.search(r'parametrize\("cfg", C\.%s\(\)' % cases.__name__, src), cases.__name__


def test_the_caps_in_the_source_are_the_caps_of_the_predicates():
    src = open(HIP).read()

    def num(pattern, text=src):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert num(r"grid_for\(size_t n, int per_block = (\d+), int cap = \d+\)") == C.THREADS
    assert num(r"grid_for\(size_t n, int per_block = \d+, int cap = (\d+)\)") == C.GRID_CAP
    launches = re.findall(r"<<<grid_for\([^;]*?\), (\d+), 0, stream>>>", src)
    assert len(launches) == len(re.findall(r"<<<grid_for\(", src)) == 5 and set(launches) == {str(C.THREADS)}     # 1 nhwc, 2 im2col, 1 bn_act, 1 maxpool: once per entry point and vector width
    assert num(r"int slabs = \(rows \+ (\d+)\) / \d+;") + 1 == C.SLAB_ROWS and num(r"int slabs = \(rows \+ \d+\) / (\d+);") == C.SLAB_ROWS
    assert num(r"if \(slabs > (\d+)\) slabs = \1;") == C.SLAB_CAP
    assert num(r"const int c = blockIdx\.x \* (\d+) \+ cg \* 4;") == C.COLS_PER_BLOCK
    assert num(r"dim3 grid\(\(C \+ (\d+)\) / \d+,") + 1 == C.COLS_PER_BLOCK and num(r"dim3 grid\(\(C \+ \d+\) / (\d+),") == C.COLS_PER_BLOCK
    assert re.search(r"dim3 grid\([^;]*\), block\(%d\);" % C.THREADS, src)
    # the row walk of col_stats that stats_walk_ends restates: 16 lanes, two rows per trip, at most one more
    assert re.search(r"for \(; r \+ 16 < r1; r \+= 32\)", src) and re.search(r"ry = threadIdx\.x >> 4;", src)
    assert re.search(r"bn_finalize_kernel<<<\(C \+ %d\) / %d, %d, 0, stream>>>" % (C.THREADS - 1, C.THREADS, C.THREADS), src)
    # the 8-wide gather's conditions
    assert "dtype == MV_BF16 && (C & 7) == 0 && (ldk & 7) == 0 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0" in src
    # sizes derived from the caps
    big = {f: [c for c in cases() if any(b.endswith("second_trip") for b in br(c))] for f, (cases, br) in C.FAMILIES.items()}
    assert all(big[f] for f in ("nhwc", "im2col", "pool", "act"))
    for c in big["nhwc"]:
        assert C.ONE_TRIP < c["B"] * c["H"] * c["W"] * c["Cp"] < 1.05 * C.ONE_TRIP, c
    for c in big["im2col"]:
        assert C.im2col_plan(c)[0] == "bf16/VEC8" and C.ONE_TRIP < C.im2col_plan(c)[3] < 1.05 * C.ONE_TRIP, c
    for c in big["pool"]:
        assert C.ONE_TRIP < C.pool_shape(c)[2] * c["C"] // 4 < 1.05 * C.ONE_TRIP, c
    for c in big["act"]:
        assert C.ONE_TRIP < c["rows"] * c["C"] // 4 < 1.05 * C.ONE_TRIP, c


def test_the_row_walk_restatement_counts_every_row_once():
    """stats_plan / stats_walk_ends against the kernel's loop written out for every row count of the sweep"""
    for rows in sorted({c["rows"] for c in C.stats_cases()} - {1050000, 1048577}) + [1025, 2000]:
        slabs, capped, rpb, gy = C.stats_plan(rows)
        seen, ends = [], set()
        for y in range(gy):
            r0, r1 = y * rpb, min(rows, y * rpb + rpb)
            for ry in range(16):
                r, last = r0 + ry, "idle"
                while r + 16 < r1:
                    seen += [r, r + 16]
                    r, last = r + 32, "pair"
                if r < r1:
                    seen.append(r)
                    last = "single"
                ends.add(last)
        assert sorted(seen) == list(range(rows)) and ends == C.stats_walk_ends(rows), rows
        assert not capped and (gy - 1) * rpb < rows <= gy * rpb
    assert C.stats_plan(1050000) == (2048, True, 513, 2047) and C.stats_plan(1048577)[1:3] == (True, 513)
    assert C.stats_plan(C.SLAB_CAP * C.SLAB_ROWS) == (2048, False, 512, 2048)


# =====================================================================================================================
# the bounds: an honest f32 restatement passes every case, each planted defect fails at least one
# =====================================================================================================================
DEFECTS = {
    "nhwc": [],
    "im2col": ["taps_transposed", "edge_padding", "tail_unwritten", "stride_after_pad"],
    "pool": ["start_at_zero", "anchor_2oy"],
    "stats": ["row_dropped", "row_doubled", "last_column_block_skipped"],
    "fin": ["biased_running_var", "momentum_on_old", "eps_outside_sqrt"],
    "act": ["residual_after_relu", "x_rounded_to_bf16_first"],
}


def _elems(cfg):
    fam = cfg["fam"]
    if fam == "nhwc":
        return cfg["B"] * cfg["H"] * cfg["W"] * cfg["Cp"]
    if fam == "im2col":
        return C.im2col_shape(cfg)[2] * cfg["ldk"]
    if fam == "pool":
        return cfg["B"] * cfg["H"] * cfg["W"] * cfg["C"]
    if fam in ("stats", "act"):
        return cfg["rows"] * cfg["C"]
    return cfg["C"]                                          # fin: C outputs, whatever the rows behind the sums


def _judge(cfg, defect=None):
    """-> (ok, worst error / bound or None): the restatement of cfg's kernel against the reference, as the GPU file judges the kernel"""
    fam = cfg["fam"]
    if fam == "nhwc":
        x = C.nhwc_inputs(cfg)
        return C.same_bits(C.nhwc_restated(x, cfg), C.nhwc_reference(x, cfg)), None
    if fam == "im2col":
        x = C.im2col_inputs(cfg)
        return C.same_bits(C.im2col_restated(x, cfg, defect), C.im2col_reference(x, cfg)), None
    if fam == "pool":
        x = C.pool_inputs(cfg)
        return C.same_bits(C.pool_restated(x, cfg, defect), C.pool_reference(x, cfg)), None
    if fam == "stats":
        x = C.stats_inputs(cfg)
        ref, bound = C.stats_reference(x, cfg)
        return C.within(C.stats_restated(x, cfg, defect), ref, bound)
    if fam == "fin":
        stats, rm, rv = C.fin_inputs(cfg)
        ref = C.fin_reference(stats, rm, rv, cfg)
        bnd = C.fin_bounds(ref, rm, rv, cfg)
        mean, rstd, nrm, nrv = C.fin_restated(stats, rm, rv, cfg, defect)
        res = [C.within(mean, ref["mean"], bnd["mean"]), C.interval_ratio(rstd, ref["rstd"], *bnd["rstd"])]
        if cfg["running"]:
            res += [C.within(nrm, ref["run_mean"], bnd["run_mean"]), C.within(nrv, ref["run_var"], bnd["run_var"])]
        return all(ok for ok, _ in res), max(r for _, r in res)
    t = C.act_inputs(cfg)
    ref, bound = C.act_reference(*t, cfg)
    return C.within(C.act_restated(*t, cfg, defect), ref, bound)


@pytest.mark.parametrize("fam", sorted(C.FAMILIES))
def test_an_honest_f32_restatement_passes_every_case(fam):
    worst = 0.0
    for cfg in C.FAMILIES[fam][0]():
        ok, ratio = _judge(cfg)
        assert ok, (cfg, ratio)
        worst = max(worst, ratio or 0.0)
    print(f"\n{fam}: honest restatement, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("fam,defect", [(f, d) for f in sorted(DEFECTS) for d in DEFECTS[f]])
def test_each_planted_defect_fails_some_case(fam, defect):
    cases = [c for c in C.FAMILIES[fam][0]() if _elems(c) <= DEFECT_MAX_ELEMS]
    caught = [c["seed"] for c in cases if not _judge(c, defect)[0]]
    print(f"\n{fam} / {defect}: caught by {len(caught)} of {len(cases)} cases")
    assert caught, (fam, defect)


def test_the_references_state_what_they_are_meant_to():
    """the written-out formulas against torch's own modules, fp64 against fp64"""
    cfg = dict(C.fin_case(16), C=7, rows=12544, running=True, momentum=0.1, eps=1e-5)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (cfg["rows"], cfg["C"]), generator=g).double()
    stats = torch.stack([x.sum(0), (x * x).sum(0)]).float()
    rm, rv = torch.randn(7, generator=g), torch.rand(7, generator=g) + 0.5
    ref = C.fin_reference(stats, rm, rv, cfg)
    bn = torch.nn.BatchNorm1d(7, eps=C.f32r(1e-5), momentum=C.f32r(0.1), dtype=torch.float64).train()
    bn.running_mean.copy_(rm)
    bn.running_var.copy_(rv)
    with torch.no_grad():
        y = bn(x)
    assert float((bn.running_mean - ref["run_mean"]).abs().max()) < 1e-12 and float((bn.running_var - ref["run_var"]).abs().max()) < 1e-12
    assert float((y - (x - ref["mean"]) * ref["rstd"]).abs().max()) < 1e-10
    one = C.fin_reference(stats, rm, rv, dict(cfg, rows=1))           # the stated rows == 1 factor: 1, not a division by zero
    assert bool(torch.isfinite(one["run_var"]).all())
    # bn_act's reference against batch_norm in eval() + residual + relu
    acfg = dict(C.act_case(3), rows=37, C=8)
    xa, mean, rstd, gamma, beta, res = C.act_inputs(acfg)
    ya, _ = C.act_reference(xa, mean, rstd, gamma, beta, res, acfg)
    var = 1.0 / rstd.double() ** 2 - 1e-3
    yb = torch.nn.functional.batch_norm(xa.double(), mean.double(), var, gamma.double(), beta.double(), False, 0.0, 1e-3)
    yb = torch.relu(yb + res.double()) if acfg["relu"] else yb + res.double()
    assert acfg["res"] and float((ya - yb).abs().max()) < 1e-10
    # half a bf16 ulp, against the encoding itself
    v = torch.tensor([1.0, 1.5, 2.0 - 2.0 ** -7, 2.0, 0.30078125, 100.0, 2.0 ** -20], dtype=torch.float64)          # exact in bf16
    nxt = (v.to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).double()
    assert torch.equal(C.half_ulp_bf16(v), (nxt - v.to(torch.bfloat16).double()) / 2)


def test_inputs_carry_what_the_checks_need():
    x = C.nhwc_inputs(C.NHWC_FIXED[0])
    r = x.to(torch.bfloat16).float()
    assert bool((r.abs() > x.abs()).any()) and bool((r.abs() < x.abs()).any())
    for v, even in ((1 + C.T8, 1.0), (1 + 3 * C.T8, 1 + 4 * C.T8)):                # the ties, both directions
        assert bool((x == v).any()) and float(torch.tensor(v).to(torch.bfloat16)) == even
    for cfg in C.pool_cases()[:C.N_POOL]:
        p = C.pool_inputs(cfg).float()
        assert bool((p < 0).all()) and not bool(torch.isnan(p).any())
        y = C.pool_reference(C.pool_inputs(cfg), cfg).float()
        assert bool(torch.isinf(y).any()), cfg                                       # some window holds nothing but -inf
    for cfg in C.act_cases()[:C.N_ACT]:
        xa, mean, rstd, gamma, beta, res = C.act_inputs(cfg)
        pre = (xa.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()
        assert bool((gamma > 0).any()) or cfg["C"] < 3
        assert bool((gamma < 0).any()) and (cfg["rows"] < 3 or (bool((pre > 0).any()) and bool((pre < 0).any()))), cfg
    for cfg in C.fin_cases():
        stats, rm, rv = C.fin_inputs(cfg)
        ref = C.fin_reference(stats, rm, rv, cfg)
        assert float(ref["var"][0]) == 0.0 and float(ref["mean"][0]) == C.FIN_CONST_VALUE, cfg
        assert torch.equal(stats.double().float(), stats) and bool((rm != 0).all()) and bool((rv != 1).all())
    xs = C.stats_inputs(C.stats_case(1))
    assert bool(torch.isnan(xs[:, C.stats_case(1)["C"]:].float()).all()) or C.stats_case(1)["ldx"] == C.stats_case(1)["C"]
