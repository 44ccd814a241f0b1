"""The grouped weight-gradient sweep on the CPU.  tests/test_gemm_grouped_sweep_gpu.py is only worth its GPU time while its cases
reach the raster's second group, n0 > 0, all-split launches, tails across problems, both bodies of the grouped reduction and every
kind of unit-to-unit transition of a block's walk; this file

* compares the plan restated in tests/gemm_grouped_cases.py, unit by unit, with the library's own (mv_gemm_grouped_fill +
  mv_gemm_grouped_decode through the C ABI, fake pointers: nothing is dereferenced),
* reads the constants of the restatement out of the .h / .hip text, so that a retune fails here instead of silently changing what is swept,
* counts what the cases reach (every named branch at least MIN_HITS times),
* shows that an honest f32 computation of every case's plan lies inside every element's bound and that each planted defect lands
  outside it in every case it applies to.

split == 8 (MV_GROUP_MAX_SPLIT) is reachable at small size -- one tile planned for 11 blocks -- so it is required like the others."""
import ctypes as C
import os
import re

import pytest
import torch

import gemm_grouped_cases as GG
from medvill_amd import _lib
from medvill_amd.hip_ops import GroupProblem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc")
GPU_FILE = os.path.join(ROOT, "tests", "test_gemm_grouped_sweep_gpu.py")
MIN_HITS = 3
P = 0x10000000      # a non-null, 256-byte aligned address that is never dereferenced
DTYPE = {GG.BF16: 1, GG.F16: 2}

REQUIRED = [
    # raster
    "n0>0", "row_group>=1", "gm=1", "gm=4", "gm=8",
    # epilogue of an unsplit unit, and what it leaves for the next unit's first wait
    "epi_all_fast", "epi_mixed_N%4", "epi_all_slow_ldc", "epi_all_slow_base", "full=1", "full=0",
    # slice units
    "slice_nonempty", "slice_empty", "slice_short",
    # the grouped reduction
    "reduce_vec", "reduce_scalar", "reduce_skip_m", "reduce_skip_n", "reduce_nsl<split",
    "reduce_vec+alpha", "reduce_vec+accumulate", "reduce_scalar+alpha", "reduce_scalar+accumulate",
    # transitions on one block
    "after_full->nst=1", "after_full->nst>1", "after_ragged->nst=1", "after_ragged->nst>1", "after_slice->nst=1", "after_slice->nst>1",
    "direct->slice", "problem_boundary", "walk>=3_units",
    # plan shapes
    "direct=0", "tail=0", "tail_in_one_problem", "tail_spans_kchunks", "split=1", "split=2", "split=3", "split=5|6", "split=8",
    "plan_blocks>launch_blocks",
    # operands
    "A_plain", "A_slice", "operands_bf16", "operands_f16",
]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _library_plan(lib, c):
    lay = GG.layout(c)
    arr = (GroupProblem * len(lay))()
    for i, p in enumerate(lay):
        base = P + 0x1000000 * 3 * i
        arr[i] = GroupProblem(base + 2 * p["a_col"], base + 0x1000000, base + 0x2000000 + 4 * p["c_off"], p["lda"], p["ldb"], p["ldc"],
                              p["No"], p["Ko"], p["rows"])
    nb = lib.mv_gemm_grouped_table_bytes(len(lay))
    buf = C.create_string_buffer(nb)
    rc = lib.mv_gemm_grouped_fill(DTYPE[c["dt"]], len(lay), arr, c["G"], buf, nb)
    assert rc == 0, (rc, GG.case_id(c))
    w = (C.c_int * (nb // 4)).from_buffer(buf)
    out = (C.c_int * 7)()
    units = []
    for u in range(w[5] + w[6] * w[7]):
        assert lib.mv_gemm_grouped_decode(buf, u, out) == 0
        units.append(tuple(out))
    entries = [dict(unit0=w[16 + 16 * i + 14], kchunk=w[16 + 16 * i + 15]) for i in range(len(lay))]
    return list(w[:16]), entries, units, lib.mv_gemm_grouped_workspace_bytes(buf)


@pytest.mark.parametrize("fam", sorted(GG.FAMILIES))
def test_the_restated_plan_is_the_librarys_plan(lib, fam):
    for c in GG.FAMILIES[fam]():
        hdr, units = GG.group_plan(c["shapes"], c["G"])
        words, entries, lib_units, ws = _library_plan(lib, c)
        assert words[3] == c["G"], GG.case_id(c)                    # every case names its block count: no plan depends on the machine
        assert words[4:8] == [hdr["units"], hdr["direct"], hdr["tail"], hdr["split"]], (GG.case_id(c), words[4:8], hdr)
        assert [e["unit0"] for e in entries] == hdr["unit0"] and [e["kchunk"] for e in entries] == hdr["kchunk"], GG.case_id(c)
        assert ws == GG.workspace_bytes(hdr), GG.case_id(c)
        assert len(units) == len(lib_units)
        for u, (mine, theirs) in enumerate(zip(units, lib_units)):
            assert mine == theirs, (GG.case_id(c), u, mine, theirs)


def test_the_plans_the_families_were_chosen_for():
    def hdr3(shapes, G):
        h = GG.group_plan(shapes, G)[0]
        return (h["direct"], h["tail"], h["split"])
    assert sum(GG.tiles_of(s) for s in GG.RASTER) == 126 and sum(GG.tiles_of(s) for s in GG.TAIL) == 9
    for G, want in zip(GG.RASTER_G, GG.RASTER_PLANS):
        assert hdr3(GG.RASTER, G) == want, G
    for G, want in zip(GG.TAIL_G, GG.TAIL_PLANS):
        assert hdr3(GG.TAIL, G) == want, G
    for layers, G, want in GG.LAYER_PLANS:
        assert hdr3(GG.LAYER * layers, G) == want, (layers, G)
    for s in GG.SPLIT8:
        assert hdr3((s,), 11) == (0, 1, 8), s
    for G in GG.WALK_G:
        assert hdr3(GG.WALK, G) == ((12, 0, 1) if G < 5 else (10, 2, 2)), G

    def tail_problems(shapes, G):
        h, units = GG.group_plan(shapes, G)
        return sorted({u[0] for u in units if u[5] >= 0}), h
    probs, h = tail_problems(GG.RASTER, 100)
    assert probs == [3, 4]
    for G in (6, 7):
        probs, h = tail_problems(GG.TAIL, G)
        assert probs == [3, 4], G
    assert (h["kchunk"][3], h["kchunk"][4]) == (64, 64)                                   # G = 7: three slices of both
    probs, h = tail_problems(GG.TAIL, 6)
    assert (h["kchunk"][3], h["kchunk"][4]) == (128, 64)                                  # G = 6: they differ
    empty = lambda shapes, G: sum(1 for u in GG.group_plan(shapes, G)[1] if u[5] >= 0 and u[3] == u[4])        # noqa: E731
    assert empty(GG.TAIL, 8) == 4 and empty(GG.TAIL, 16) == 3
    # every family holds what the sweep was asked to hold
    assert {c["dt"] for c in GG.raster_cases()} == {GG.BF16, GG.F16}
    assert {c["shapes"] for c in GG.raster_cases() if c["single"]} == {(s,) for s in GG.RASTER}
    assert all(c["G"] == GG.tiles_of(c["shapes"][0]) for c in GG.raster_cases() if c["single"])
    assert {c["G"] for c in GG.raster_cases() if not c["single"]} == set(GG.RASTER_G)
    wk = GG.walk_cases()
    assert all(c["launches"] == 2 and len(c["shapes"]) >= 7 for c in wk) and len({c["shapes"] for c in wk}) >= 2 and {c["G"] for c in wk} >= {1, 2, 3}
    tl = [c for c in GG.tail_cases() if c["shapes"] == GG.TAIL]
    assert {(c["G"], c["alpha"], c["accumulate"], c["cplace"][3]) for c in tl} == \
        {(G, al, acc, p) for G in GG.TAIL_G for al in (None, GG.ALPHA) for acc in (0, 1) for p in GG.CPLACE}
    assert {c["cplace"][4] for c in tl} == set(GG.CPLACE)
    assert all(c["alpha"] is not None and c["aform"][2] == "slice" and c["shapes"][3] == (2304, 768, 136) for c in GG.layer_cases())
    assert {(c["G"], c["pcus"]) for c in GG.grid_cases()} == {(16, (0, 3)), (3, (0, 2))}
    assert max(r for c in GG.all_cases() for _, _, r in c["shapes"]) <= 448


def test_the_constants_in_the_source_are_the_constants_of_the_restatement():
    grp, ring, tn, gemm = _src("mv_gemm_group.h"), _src("mv_gemm_ring.h"), _src("mv_gemm_ring_tn.hip"), _src("mv_gemm.hip")

    def num(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert num(grp, r"#define MV_GROUP_MAX_SPLIT (\d+)") == GG.MAX_SPLIT
    assert num(grp, r"#define MV_GROUP_TILE (\d+)") == GG.TILE
    assert num(grp, r"#define MV_GROUP_BK (\d+)") == GG.BK
    m = re.search(r"if \((\d+) \* n >= (\d+) \* rounds \* G\) return s;", grp)
    assert m and (int(m.group(1)), int(m.group(2))) == (GG.FILL_DEN, GG.FILL_NUM)
    assert "for (int s = 1; s <= MV_GROUP_MAX_SPLIT; ++s)" in grp
    assert num(grp, r"const int GM = (\d+), per_group = GM \* tiles_n;") == GG.GM
    assert "const int q = n >> 3, r = n & 7, xcd = u & 7, in = u >> 3;" in grp and GG.XCDS == 8
    assert "h.tail = h.split > 1 ? rem : 0;" in grp and "kc = (kc + MV_GROUP_BK - 1) / MV_GROUP_BK * MV_GROUP_BK;" in grp
    kern = ring[ring.index("void gemm_pring_grouped_kernel("):ring.index("// Launch of the ring kernel a plan names")]
    assert num(kern, r"constexpr int EPI_OPS = (\d+);") == GG.EPI_OPS
    # what unit_state() restates: the one-stage floor, vec_ok, full, and what either kind of unit leaves in epi_ops
    assert kern.count("max(1, (d.kend - d.kbeg + BKS - 1) / BKS)") == 2
    assert "p.vec_ok = ((p.ldc & 3) == 0) && ((((uintptr_t)p.C) & 15) == 0);" in kern
    assert "const bool full = (m0 + G2_BM <= p.M) && (n0 + BN <= p.N) && ((p.N & 3) == 0) && p.vec_ok;" in kern
    assert "epi_ops = full ? EPI_OPS : 0;" in kern and "epi_ops = EPI_OPS;" in kern
    assert "LAUNCH" not in kern and "gemm_pring_grouped_kernel<4, 4, 2, true>" in tn and "gemm_pring_grouped_kernel<4, 4, 2, false>" in tn      # NSTAGE = 2
    red = tn[tn.index("void splitk_reduce_grouped_kernel("):tn.index("int mv_launch_ring_tn_grouped(")]
    assert "const bool vec = ((ldc & 3) == 0) && ((((uintptr_t)C) & 15) == 0) && ((N & 3) == 0);" in red
    assert "const int nsl = (e->K + e->kchunk - 1) / e->kchunk;" in red and "if (m >= M || n >= N) continue;" in red
    assert "const int n_max = mv_persistent_blocks(gemm_knobs().persistent_cus, gemm_n_cu());" in gemm and "const int n_blk = h.n_blocks < n_max ? h.n_blocks : n_max;" in gemm
    assert "const dim3 grid(units < n_blk ? units : n_blk), block(512);" in tn


def test_every_named_branch_is_reached():
    count = GG.census()
    for fam in GG.FAMILIES:
        print(f"\n{fam}: {len(GG.FAMILIES[fam]())} cases")
    per_fam = {fam: GG.census(fam) for fam in GG.FAMILIES}
    for name in sorted(set(REQUIRED) | set(count)):
        where = ", ".join("%s %d" % (f, per_fam[f][name]) for f in GG.FAMILIES if name in per_fam[f])
        print(f"    {name:32s} {count.get(name, 0):4d}{'' if name in REQUIRED else '   (not required)'}   [{where}]")
    short = {n: count.get(n, 0) for n in REQUIRED if count.get(n, 0) < MIN_HITS}
    assert not short, f"reached by fewer than {MIN_HITS} cases: {short}"


def test_generated_cases_are_inside_the_abi_and_poisoned():
    for c in GG.all_cases():
        assert c["dt"] in DTYPE and len(c["shapes"]) <= 256
        for p in GG.group_inputs(c):
            No, Ko, rows = p["No"], p["Ko"], p["rows"]
            assert p["lda"] % 8 == 0 and p["ldb"] % 8 == 0 and p["a_col"] % 8 == 0 and p["lda"] >= p["a_col"] + No and p["ldb"] >= Ko and p["ldc"] >= Ko
            A, B = p["A"].float(), p["B"].float()
            assert A.shape == (rows + GG.GUARD_ROWS, p["lda"]) and B.shape == (rows + GG.GUARD_ROWS, p["ldb"])
            for st, col, width in ((A, p["a_col"], No), (B, 0, Ko)):
                assert bool(torch.isfinite(st[:rows, col:col + width]).all()), GG.case_id(c)
                assert bool(torch.isnan(st[:rows, :col]).all()) and bool(torch.isnan(st[:rows, col + width:]).all()) and bool(torch.isnan(st[rows:]).all())
            assert torch.equal(A[:rows, p["a_col"]:p["a_col"] + No], p["a"].float().t()) and torch.equal(B[:rows, :Ko], p["b"].float().t())
            flat, win = GG.c_buffer(p)
            assert bool(torch.isnan(win[:No, Ko:]).all()) and bool(torch.isnan(win[No:]).all()) and bool(torch.isnan(flat[:p["c_off"]]).all())
            assert (p["C0"] is not None) == bool(c["accumulate"])
            if p["C0"] is not None:
                assert float(p["C0"].std()) > 0.5                   # a random C0, not a constant


def test_the_gpu_file_cannot_drop_a_case():
    import ast
    src = open(GPU_FILE).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
    for gen in GG.FAMILIES.values():
        assert re.search(r'parametrize\("cfg", GG\.%s\(\)' % gen.__name__, src), gen.__name__


# ---- the bounds let an honest f32 computation through and catch every planted defect ------------------------------------------------
_CACHE = {}


def _evaluated(c):
    key = GG.case_id(c) + repr(c["cplace"])
    if key not in _CACHE:
        t = GG.group_inputs(c)
        _CACHE[key] = (t, GG.group_reference(c, t))
    return _CACHE[key]


def _worst(c, defect=None):
    t, ref = _evaluated(c)
    worst = 0.0
    for got, (r, bound) in zip(GG.honest_group(c, t, defect), ref):
        ok, w = GG.within(got, r, bound)
        worst = max(worst, w if ok or w > 1 else float("inf"))
    return worst


def test_an_honest_f32_computation_passes_every_bound():
    worst, at = 0.0, None
    for c in GG.all_cases():
        w = _worst(c)
        if w > worst:
            worst, at = w, c
        assert w <= 1.0, (w, GG.case_id(c), c)
    print(f"\nhonest f32 computation: worst error / bound = {worst:.3f} at {GG.case_id(at)}")
    assert worst > 0.001, "bounds this loose could not see a defect"


@pytest.mark.parametrize("defect", GG.DEFECTS)
def test_every_planted_defect_fails_the_bound_of_every_case_it_applies_to(defect):
    cases = [c for c in GG.all_cases() if GG.defect_applies(defect, c)]
    assert len(cases) >= 10, (defect, len(cases))
    figures = [(_worst(c, defect), GG.case_id(c)) for c in cases]
    print(f"\n{defect}: {len(cases)} cases, smallest error / bound under the defect = {min(figures)[0]:.1f}")
    passed = [i for w, i in figures if w <= 1.0]
    assert not passed, f"{defect}: not caught in {passed}"


def test_reference_equals_loops_over_the_stored_operands():
    """the reference works on the logical operands; here the product is rebuilt from the STORAGE the kernel is given (column slice of the
    wide buffer, leading dimensions), for one small table"""
    c = GG.base("tail", 7, ((9, 5, 11), (8, 6, 3)), 2, aform=("plain", "slice"), alpha=GG.ALPHA, accumulate=1)
    t = GG.group_inputs(c)
    for p, (ref, _) in zip(t, GG.group_reference(c, t)):
        A, B = p["A"].double(), p["B"].double()
        y = torch.zeros((p["No"], p["Ko"]), dtype=torch.float64)
        for m in range(p["No"]):
            for n in range(p["Ko"]):
                for k in range(p["rows"]):
                    y[m, n] += A[k, p["a_col"] + m] * B[k, n]
        want = y * float(torch.tensor(GG.ALPHA, dtype=torch.float32)) + p["C0"].double()
        assert float((ref - want).abs().max()) <= 1e-12
