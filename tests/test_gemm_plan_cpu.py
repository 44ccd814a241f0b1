"""mv_gemm's launch plan (csrc/mv_gemm_plan.h) against its restatement gemm_cases.plan(), on the CPU.

The planner is plain host C++; tests/native/gemm_plan_check.cpp reads calls from stdin and prints their plans.  This file compiles it
once with the host C++ compiler (no compiler is a failure: the library cannot be built without one either), feeds it

* every case of G.all_gemm_cases() under its own knobs, at 256 CUs and at 304, and
* a grid built from the named thresholds of the header: for every threshold the governing dimension at T - 1, T, T + 1 with the other
  dimensions on both sides of theirs, every such shape on the four layouts and the three operand encodings,

and compares every field both sides have: kernel, variant, rule, tiles, sk_auto, slabs, kchunk, the persistent form's blocks, whether the
reduce follows, and the refusal code (restated here from mv_gemm's checks).

The other axes of the grid -- splitk {-1, 0, 1, 2, 7, 40}, the four workspace modes, force {0, 1, 2}, nj {0, 14, 24, 10, 2, 4, 32 and the
undocumented 7}, rounds {0, 1}, impl {0, 1}, column sums on / off, CU counts {256, 304, 100 (no multiple of 8)} -- have 165,888
combinations per (shape, layout, encoding); their full product over ~2,700 of those is 4 x 10^8 plans, hours of the Python restatement.
The grid therefore takes every (shape, layout, encoding) with DRAWS combinations drawn from that product by a fixed generator (weighted: half of
the draws keep force = nj = 0, where the automatic route's rules apply; column sums, which most calls are refused with, in one draw of
four; impl = 1, which switches everything else off, in one of six), and asserts that every value of every axis, every kernel and every rule of the
route are among the accepted calls."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc", "mv_gemm_plan.h")
PROGRAM = os.path.join(ROOT, "tests", "native", "gemm_plan_check.cpp")
OK, E_ARG, E_SHAPE, E_DTYPE, E_WORKSPACE = 0, -1, -2, -3, -4            # include/medvill.h
DT_CODE = {G.F32: 0, G.BF16: 1, G.F16: 2}
KERNELS = ["valu", "mfma128", "mfma128_2stage", "ring14", "pring", "ring320", "ring256x128", "ring_tn4"]          # enum MvGemmKernel
RULES = ["plain", "rounds256", "rounds320", "rounds_back_to_128", "wide320", "wide256"]                           # enum MvGemmRule
FIELDS = ["rc", "kernel", "variant", "rule", "tiles", "sk_auto", "splitk", "kchunk", "grid_x", "grid_y", "grid_z", "block", "lds_bytes", "units",
          "blocks", "reduce", "ring_lds_ok"]
SPLITKS, WS_MODES, FORCES, NJS, CUS = (-1, 0, 1, 2, 7, 40), ("none", "exact", "short", "ample"), (0, 1, 2), (0, 14, 24, 10, 2, 4, 32, 7), (256, 304, 100)
DRAWS = 16


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (CXX, c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", PROGRAM, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def call_line(c, n_cu):
    fl, wsf = G.flags(c), G.ws_floats(c, n_cu)
    v = [DT_CODE[c["dt"]], c["ta"], c["tb"], c["M"], c["N"], c["K"], c["splitk"], 4 * max(wsf or 0, 0), int(wsf is not None), c["epi"], DT_CODE[c["cdt"]],
         c["accumulate"], int(c["c3dt"] is not None), int(c["csum"]), int(fl["vec8_ok"]), int(bool(fl["r8_ok"])), int(c["alpha"] is not None),
         int(c["p_drop"] > 0), 1, c["impl"], c["force"], c["nj"], c["rounds"], c["pcus"], n_cu]
    return " ".join(str(int(x)) for x in v)


def run(program, points):
    """points: [(cfg, n_cu)] -> one dict of the plan's fields per point"""
    text = "\n".join(call_line(c, n) for c, n in points) + "\n"
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, len(FIELDS))
    assert len(rows) == len(points)
    return [dict(zip(FIELDS, (int(x) for x in row))) for row in rows]


def expected_rc(c, pl, n_cu):
    """the refusals of mv_gemm that the planner owns, in its order (the pointer and leading-dimension checks come before the plan)"""
    M, N, epi = c["M"], c["N"], c["epi"]
    fl, wsf = G.flags(c), G.ws_floats(c, n_cu)
    sk = c["splitk"] if c["splitk"] >= 0 else 1
    plain = epi == G.EPI_NONE and c["cdt"] == G.F32 and not c["c3dt"]
    mfma = c["dt"] != G.F32 and c["impl"] == 0
    if (sk > 1 or c["accumulate"]) and not plain:
        return E_SHAPE
    if sk > 1 and (wsf is None or max(wsf, 0) < sk * M * N):
        return E_WORKSPACE
    if c["alpha"] is not None and not plain:
        return E_ARG
    if c["p_drop"] > 0 and N % 4:
        return E_SHAPE
    if mfma and c["dt"] == G.F16 and c["ta"] and not c["tb"]:
        return E_DTYPE
    if c["csum"]:
        ring = pl["kernel"] in G.RING_TILE
        if not (ring and pl["variant"] == 14 and pl["slabs"] == 1 and not c["accumulate"] and fl["vec8_ok"] and N % 256 == 0 and c["cdt"] != G.F32
                and (epi in G.WIDE_E or (epi in (G.EPI_MUL, G.EPI_RES) and fl["r8_ok"]))):
            return E_SHAPE
    if not mfma and G.cdiv(M, G.VALU_TILE) > 65535:
        return E_SHAPE
    return OK


def compare(c, n_cu, got):
    """-> (kernel, rule) when the call is accepted, else None"""
    pl = G.plan(c, n_cu)
    where = (c, n_cu, got, {k: pl.get(k) for k in ("kernel", "variant", "rule", "tiles", "sk_auto", "slabs", "kchunk")})
    assert got["rc"] == expected_rc(c, pl, n_cu), where
    # the route is the same whether or not the call is then refused (f16 operands of A^T.B^T have no kernel to name)
    assert (got["variant"], RULES[got["rule"]]) == (pl["variant"], pl["rule"]), where
    assert KERNELS[got["kernel"]] == pl["kernel"] or (c["dt"] == G.F16 and c["ta"] and not c["tb"]), where
    if "tiles" in pl:
        assert (got["tiles"], got["sk_auto"]) == (pl["tiles"], pl["sk_auto"]), where
    if got["rc"] != OK:
        return None
    assert (got["splitk"], got["kchunk"], got["reduce"]) == (pl["slabs"], pl["kchunk"], int(pl["slabs"] > 1)), where
    assert got["ring_lds_ok"] == 1, where
    if pl["kernel"] == "pring":
        units = G.cdiv(c["M"], 256) * G.cdiv(c["N"], 256) * pl["slabs"]
        blocks = min(units, c["pcus"] if 0 < c["pcus"] < n_cu else n_cu)
        assert (got["units"], got["blocks"], got["grid_x"], got["grid_y"]) == (units, blocks, blocks, 1) and units / blocks == pl["units_per_block"], where
    elif pl["kernel"] == "valu":
        assert (got["grid_x"], got["grid_y"], got["grid_z"], got["lds_bytes"]) == (G.cdiv(c["N"], 64), G.cdiv(c["M"], 64), pl["slabs"], 0), where
    else:
        bm, bn, bk = pl["tile"]
        assert (got["grid_x"], got["grid_y"], got["grid_z"]) == (G.cdiv(c["M"], bm) * G.cdiv(c["N"], bn), pl["slabs"], 1), where
        stages = G.RING_STAGES.get(pl["kernel"], 2 if pl["kernel"] == "mfma128_2stage" else 1)
        assert got["lds_bytes"] == stages * (bm + bn) * bk * 2 and got["block"] == (256 if bn == 128 else 512), where
    return pl["kernel"], pl["rule"]


def threshold_shapes():
    """(M, N, K): for every threshold of mv_gemm_plan.h the dimension that governs it at T - 1, T, T + 1, the others on both sides of theirs"""
    def around(t):
        return (t - 1, t, t + 1)
    S = set()

    def add(Ms, Ns, Ks):
        S.update((m, n, k) for m in Ms for n in Ns for k in Ks)
    rows_for_t128 = 256 * G.BIG_MIN_T128
    add(around(G.BIG_MIN_M), (120, 136, 2048), (64, 8192))
    add((200, 264, rows_for_t128), around(G.BIG_MIN_N), (64, 8192))
    add((256,), tuple(128 * t for t in around(G.BIG_MIN_T128)) + (128 * G.BIG_MIN_T128 + 1,), (64, 8192))           # 256 x 128 tiles: 127, 128, 129
    add(tuple(256 * t for t in around(G.BIG_MIN_T128)) + (rows_for_t128 + 1,), (128, 1024), (64, 8192))
    add((200, 512), (100, 256, 1024), around(G.BIG_LONG_K) + (G.BIG_LONG_K - 8, G.BIG_LONG_K + 8))
    add((255, 4096, rows_for_t128), around(G.WIDE_NT_MIN_N) + (1016, 1032), (64, 8192))
    add(around(G.ROUNDS_MIN_M) + (21761,), (248, 768, 3072), (248, 512))
    add((2040, 4224, 21761), around(G.ROUNDS_MIN_N) + (248, 264), (248, 512))
    add((2040, 4224, 21761), (248, 768), around(G.ROUNDS_MIN_K) + (248, 264))
    # the two cost tables: shapes whose whole-rounds costs differ by one round between the tile heights (AUTO_TABLE) and their neighbours in M
    for m, n, k, *_ in G.AUTO_TABLE:
        add((m - 1, m, m + 1), (n,), (k,))
    add(tuple(128 * t for t in around(G.SLOTS_128)) + (128 * G.SLOTS_128 + 1,), (128,), (G.SK_MIN_K - 1, 4096))      # 128 x 128 tiles: 511, 512, 513
    add(tuple(256 * t for t in around(G.SLOTS_RING)) + (256 * G.SLOTS_RING + 1,), (256,), (G.SK_MIN_K - 1, 4096))
    add(tuple(256 * t for t in around(G.SLOTS_RING_V128)) + (256 * G.SLOTS_RING_V128 + 1,), (128,), (G.SK_MIN_K - 1, 4096))
    add((256, 512), (128, 256), around(G.SK_MIN_K) + around(3 * G.SK_DEPTH))
    add((128, 256), (128, 256), around(G.SK_CAP_128 * G.SK_DEPTH))
    add((256, 512), (128, 256), around(G.SK_CAP_RING * G.SK_DEPTH))
    add((64 * 65535 - 1, 64 * 65535, 64 * 65535 + 1), (4,), (8,))                                                    # VALU: grid.y at 65535, 65536
    return sorted(S)


def grid_points():
    rs = np.random.RandomState(20250)
    pts, seed = [], 0
    for M, N, K in threshold_shapes():
        for lay, (ta, tb) in G.LAYOUTS.items():
            for dt in (G.BF16, G.F16, G.F32):
                for _ in range(DRAWS):
                    csum = rs.randint(4) == 0
                    auto = rs.randint(2) == 0          # half of the draws leave force and nj alone: the rules of the automatic route need both at 0
                    c = G.base("plan_grid", seed, dt=dt, ta=ta, tb=tb, M=M, N=N, K=K, splitk=int(SPLITKS[rs.randint(6)]), ws=WS_MODES[rs.randint(4)],
                               force=0 if auto else int(FORCES[rs.randint(3)]), nj=0 if auto else int(NJS[rs.randint(8)]), rounds=int(rs.randint(2)), impl=int(rs.randint(6) == 0),
                               csum=csum, cdt=G.BF16 if csum else G.F32)
                    pts.append((c, int(CUS[rs.randint(3)])))
                    seed += 1
    return pts


def test_the_plan_is_the_restated_plan(program):
    cases = [(c, n) for n in (256, 304) for c in G.all_gemm_cases()]
    grid = grid_points()
    plans = run(program, cases + grid)
    reached, accepted = {}, 0
    for (c, n), got in zip(cases, plans):          # (at another CU count the automatic route of a column-sum case may be one that refuses it)
        assert got["rc"] == OK or n != G.DEFAULT_CUS, (c, n, got)
    seen = {k: set() for k in ("splitk", "ws", "force", "nj", "rounds", "impl", "csum", "n_cu")}
    for (c, n), got in zip(cases + grid, plans):
        hit = compare(c, n, got)
        if hit:
            accepted += 1
            reached[hit] = reached.get(hit, 0) + 1
            for k in seen:
                seen[k].add(n if k == "n_cu" else c[k])
    print(f"\n{len(cases)} case plans + {len(grid)} grid plans compared ({len(threshold_shapes())} shapes), {accepted} accepted; "
          f"{len(reached)} distinct (kernel, rule) pairs:")
    for k in sorted(reached):
        print(f"    {k[0]:16s} {k[1]:20s} {reached[k]:6d}")
    assert {k for k, _ in reached} == set(KERNELS), sorted(set(KERNELS) - {k for k, _ in reached})
    assert {r for _, r in reached} == set(RULES), sorted(set(RULES) - {r for _, r in reached})
    assert seen["splitk"] >= set(SPLITKS) and seen["ws"] >= set(WS_MODES) and seen["force"] >= set(FORCES) and seen["nj"] >= set(NJS)
    assert seen["rounds"] >= {0, 1} and seen["impl"] >= {0, 1} and seen["csum"] >= {False, True} and seen["n_cu"] >= set(CUS)


def test_workspace_bytes_is_the_plans_wish(program):
    """mv_gemm_workspace_bytes asks the plan with splitk = 0 and nothing else set (csrc/mv_gemm.hip)"""
    cases = [(dict(c, splitk=0, ws="none", epi=G.EPI_NONE, cdt=G.F32, rdt=None, c3dt=None, accumulate=0, alpha=None, p_drop=0.0, csum=False), n)
             for n in (256, 100) for c in G.all_gemm_cases()]
    for (c, n), got in zip(cases, run(program, cases)):
        bytes_ = got["sk_auto"] * c["M"] * c["N"] * 4 if got["sk_auto"] > 1 else 0
        assert bytes_ == G.workspace_bytes(c, n), (c, n, got)


def test_the_ring_shapes_are_the_tiles_of_the_restatement():
    src = open(PLAN_H).read()
    for name, (bm, bn, bk) in G.RING_TILE.items():
        enum = {"ring14": "MvRingShape{4, 4, 2, 2, 8}", "pring": "MvRingShape{4, 4, 2, 2, 8}", "ring320": "MvRingShape{4, 4, 2, 2, 10}",
                "ring256x128": "MvRingShape{4, 2, 3, 1, 8}", "ring_tn4": "MvRingShape{4, 4, 4, 1, 8}"}[name]
        nj, wn, nstage, ks, mi = (int(x) for x in enum[enum.index("{") + 1:-1].split(","))
        assert enum in src and (32 * mi, wn * 16 * nj, G.G2_BK * ks, nstage) == (bm, bn, bk, G.RING_STAGES[name]), name
