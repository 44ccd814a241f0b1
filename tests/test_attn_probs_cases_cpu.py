"""Census of the attention-probability sweep (CPU).  tests/test_attn_probs_sweep_gpu.py is only worth its GPU time while its cases
reach every branch of mv_attn_probs; this file counts the branches from the dense masks, checks the constants the restatement relies on
against csrc/mv_attn*.{h,hip}, shows that the fp64 reference alone passes every assertion of the sweep, and validates the bound of
tests/attn_probs_cases.py with a torch stand-in: the honest one stays within the bound on every case, seven deliberately wrong ones
each break it."""
import ast
import os
import re
import sys
from collections import Counter

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import attn_cases as C                        # noqa: E402
import attn_probs_cases as P                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE = os.path.join(ROOT, "tests", "test_attn_probs_sweep_gpu.py")
MIN_HITS = 3


def _entry_body(src):
    i = src.index('extern "C" int mv_attn_probs(')
    return src[i:]


def test_every_named_branch_is_reached():
    total = Counter()
    for c in P.all_cases():
        total.update(set(P.dispatch(c)))
    for name in sorted(set(P.BRANCHES) | set(total)):
        print(f"    {name:24s} {total.get(name, 0):4d}")
    short = {n: total.get(n, 0) for n in P.BRANCHES if total.get(n, 0) < MIN_HITS}
    assert not short, f"branches reached by fewer than {MIN_HITS} cases: {short}"
    assert set(total) <= set(P.BRANCHES)


def test_every_length_family_kind_and_option_is_drawn():
    cases = P.all_cases()
    mf = [c for c in cases if c["path"] == "mfma"]
    va = [c for c in cases if c["path"] == "valu"]
    assert {c["L"] for c in mf} >= set(C.LENGTHS) and max(c["L"] for c in cases) == 577
    assert {(c["B"], c["A"]) for c in mf if c["L"] < 321} >= set(C._BA)
    fams = {f for c in mf if c["mask"]["kind"] == "family" for f in c["mask"]["fam"]}
    assert fams == set(C.FAMILY_ID)
    assert {c["mask"]["kind"] for c in mf} == set(C.DENSE_KINDS) | {"family"}
    for enc in (C.BF16, C.F16):
        sub = [c for c in mf if c["enc"] == enc]
        assert {(c["p"], c["out"] == C.F32, c["hm"]) for c in sub} == {(p, o, h) for p in (0.0, 0.1) for o in (True, False) for h in (0, 1)}, enc
    assert {(c["enc"], c["dh"]) for c in va} == {(e, d) for e in (C.F32, C.BF16, C.F16) for d in C.VALU_DH}
    assert {c["hm"] for c in va} == {0, 1} and {c["p"] for c in va} == {0.0, 0.1}
    for c in cases:                                # dense rows only, inside the ABI
        assert not c.get("lens") and not c.get("qlim"), c
        assert (c["L"] + 63) // 64 <= P.MAX_T and c["dh"] <= P.VALU_MAX_DH and (c["path"] != "mfma" or c["dh"] == P.MFMA_DH), c
        assert c["out"] in (C.F32, c["enc"]), c


def test_constants_match_the_source():
    src = C.attn_source()
    body = _entry_body(src)
    assert int(re.search(r"if \(Tt > (\d+)\) return MV_E_SHAPE;", body).group(1)) == P.MAX_T
    assert int(re.search(r"if \(dh != (\d+)\) return MV_E_SHAPE;", body).group(1)) == P.MFMA_DH
    assert int(re.search(r"if \(dh > (\d+)\) return MV_E_SHAPE;", body).group(1)) == P.VALU_MAX_DH
    m = re.search(r"a\.vec = \(L % \(o32 \? (\d+) : (\d+)\)\) == 0;", body)
    assert (int(m.group(1)), int(m.group(2))) == (P.VEC_MULTIPLE[4], P.VEC_MULTIPLE[2])
    assert int(re.search(r"#define ATT_PATCH_BYTES (\d+)", src).group(1)) == P.PATCH_BYTES == 32 * 144
    assert float(re.search(r"#define MASK_ADD \((-?[\d.]+)f\)", src).group(1)) == C.MASK_ADD
    assert "for (int tk = wid >> 1; tk < T; tk += 2)" in src                  # key tiles by parity of the wave pair (keypar0 / keypar1)
    assert "const int q0 = tq * 64 + 32 * (wid & 1)" in src and "if (q0 >= L) return;" in src
    assert re.search(r"g_mv_impl == 0\) \{\s*if \(dh != 64\)", body)           # the impl knob routes 16-bit data to the VALU kernel
    assert "mv_debug" not in body and "MV_KNOB_COUNT = 10" in open(os.path.join(C.CSRC, "mv_common.h")).read()   # no new knob


def _one(cfg):
    qkv, _ = C.inputs(cfg)
    dense, keep = C.dense_mask(cfg), C.cpu_keep(cfg)
    R = P.reference(cfg, qkv.double(), dense, keep)
    return qkv, dense, keep, R


@pytest.fixture(scope="module")
def prepared():
    return [(c,) + _one(c) for c in P.all_cases()]


def test_the_fp64_reference_alone_passes_every_assertion(prepared):
    """the grading of the GPU file applied to the reference rounded to the output encoding: no case may fail on the harness itself"""
    assert len(prepared) == P.N_FAMILY + P.N_DENSE + P.N_VALU
    for c, qkv, dense, keep, R in prepared:
        got = R["ref"].to(C.DT[c["out"]])
        r = P.grade(c, got, R)
        assert r <= 0.5, (c, r)                    # a rounding of the exact value: half of the bound at most (SAFETY = 2)


def test_the_honest_stand_in_stays_within_the_bound(prepared):
    worst = {}
    for c, qkv, dense, keep, R in prepared:
        got = P.standin(c, qkv, dense, keep, R["lse32"])
        r = P.grade(c, got, R)
        key = (c["path"], c["enc"], c["out"], c["hm"])
        if r > worst.get(key, (0.0, None))[0]:
            worst[key] = (r, P.case_id(c))
    for key in sorted(worst):
        print(f"    stand-in {key} worst error / bound {worst[key][0]:.3f}   ({worst[key][1]})")
    assert all(v[0] <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("bug", P.BUGS)
def test_a_planted_defect_breaks_the_bound(prepared, bug):
    hits = 0
    for c, qkv, dense, keep, R in prepared:
        if P.worst(c, P.standin(c, qkv, dense, keep, R["lse32"], bug), R) > 1.0:
            hits += 1
            if hits >= 3:
                break
    assert hits >= 3, (bug, hits)


def test_the_gpu_file_iterates_every_generator_and_skips_nothing():
    src = open(GPU_FILE).read()
    tree = ast.parse(src)
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
              and isinstance(n.func.value, ast.Name) and n.func.value.id == "P"}
    assert {"family_cases", "dense_cases", "valu_cases", "grade", "reference"} <= called, called
    assert "skip" not in src and "xfail" not in src
