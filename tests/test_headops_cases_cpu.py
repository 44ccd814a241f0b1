"""Branch census and bound check of the sweep of the fine-tuning loss and optimizer kernels (CPU).  tests/test_headops_sweep_gpu.py is
only worth its GPU time while its cases reach every branch of csrc/mv_lmloss.hip, csrc/mv_vqa.hip and csrc/mv_optim.hip and its bounds
can tell a right kernel from a wrong one; this file counts the branches, checks the caps the predicates rely on against the .hip
sources, checks that every case lies inside the ABI and that the GPU file cannot drop one, and runs an honest f32 restatement of
every kernel, and the same restatement with one defect planted at a time, through the very references, bounds and judgement the GPU
file applies."""
import ast
import math
import os
import re

import numpy as np
import pytest
import torch

import headops_cases as C
import report_finetune_cases as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc")
GPU_FILE = os.path.join(ROOT, "tests", "test_headops_sweep_gpu.py")

REQUIRED = {
    "lmf": ["lmf_vec", "lmf_scalar:ld%4", "lmf_scalar:base+1float", "lmf_one_trip", "lmf_trips>1", "lmf_V%4==0", "lmf_V%4==1", "lmf_V%4==2",
            "lmf_V%4==3", "lmf_pad_columns", "lmf_ld==V", "lmf_ls=0", "lmf_ls=0.1", "lmf_ls=1", "lmf_hit_given", "lmf_hit_null", "lmf_V<256",
            "lmf_V>=256", "lmf_label0_ls=0", "lmf_label0_ls=0.1", "lmf_label0_ls=1", "lmf_label_1", "lmf_label_V-1",
            "lmf_label_in_last_partial_vector", "lmf_entries=0", "lmf_entries=1", "lmf_entries=3", "lmf_entries=300"]
           + ["lmf_row_" + p for p in C.LMF_PATTERNS],
    "lms": ["lms_B<=256", "lms_sample_trips>1", "lms_B=cap", "lms_k=0", "lms_k=1", "lms_k=B-1", "lms_k=B", "lms_n=0", "lms_sample_without_entries",
            "lms_zero_weight_with_hit", "lms_zero_weight_without_hit", "lms_hit_given", "lms_hit_null", "lms_exact_ties"],
    "lmb": ["lmb_d_f32", "lmb_d_bf16", "lmb_d_f16", "lmb_vec", "lmb_vec:d_base+8B", "lmb_scalar:ld%4", "lmb_scalar:ldd%4", "lmb_scalar:logits_base",
            "lmb_scalar:d_base", "lmb_ldd==V", "lmb_ldd==up(V,4)", "lmb_ldd==ld", "lmb_ldd==ld+8", "lmb_ldd!=ld", "lmb_one_trip", "lmb_trips>1",
            "lmb_loss_scale_given", "lmb_loss_scale_null", "lmb_ls=0", "lmb_ls=0.1", "lmb_ls=1", "lmb_!any:noentry", "lmb_!any:alldropped",
            "lmb_!any:allzeroweight", "lmb_!any:alllabel0", "lmb_row_mixed", "lmb_row_same3", "lmb_row_two_in_vec", "lmb_label_0_plain",
            "lmb_label_0", "lmb_label_1", "lmb_label_V-1", "lmb_label_1023", "lmb_label_1024", "lmb_label>1024"],
    "lmchain": ["lmchain_vec", "lmchain_scalar", "lmchain_d_f32", "lmchain_d_bf16", "lmchain_d_f16", "lmchain_ls=0", "lmchain_ls=0.1", "lmchain_ls=1"],
    "bce": ["bce_A<=256", "bce_second_trip", "bce_idle_threads", "bce_no_idle_thread", "bce_A==1_infer_fallback", "bce_inference", "bce_all_outputs",
            "bce_no_stats", "bce_no_arg_train", "bce_no_arg_infer", "bce_d_none", "bce_d_f32", "bce_d_bf16", "bce_d_f16", "bce_ldd>A", "bce_ldd==A",
            "bce_gs_host", "bce_gs_dev", "bce_ls_given", "bce_ls_null", "bce_ans_type_0/1/2", "bce_ans_type_absent", "bce_ld-A=0", "bce_ld-A=1",
            "bce_ld-A=6"] + ["bce_tie_" + t for t in C.BCE_TIES] + ["bce_" + p for p in C.BCE_PATTERNS],
    "bceml": ["bceml_C<64", "bceml_C==64", "bceml_second_trip", "bceml_inference", "bceml_all_outputs", "bceml_no_loss", "bceml_no_dgrad",
              "bceml_no_probs", "bceml_no_counters", "bceml_d_f32", "bceml_d_bf16", "bceml_d_f16", "bceml_ldd>C", "bceml_ldd==C", "bceml_ld>C",
              "bceml_ld==C", "bceml_gs_host", "bceml_gs_dev", "bceml_ls_given", "bceml_ls_null", "bceml_two_calls", "bceml_edges", "bceml_sat",
              "bceml_gauss"] + ["bceml_pw_" + p for p in C.BCEML_PW],
    "rmul": ["rmul_f32", "rmul_bf16", "rmul_f16", "rmul_one_trip", "rmul_trips>1", "rmul_partial_last_trip", "rmul_whole_trips", "rmul_ld>H",
             "rmul_ld==H", "rmul_same_buffer", "rmul_two_buffers", "rmul_idle_waves", "rmul_full_blocks", "rmul_blocks>1", "rmul_one_block"]
            + ["rmul_neg_" + n for n in C.RMUL_NEG],
    "optim": ["optim_count=%d" % c for c in C.OPTIM_COUNTS] + ["optim_T=1", "optim_T=12", "optim_tail_1", "optim_tail_2", "optim_tail_3",
              "optim_whole_vectors", "optim_decay_on", "optim_decay_off", "optim_chunks=1", "optim_chunks=2", "optim_chunks=3",
              "optim_inactive_none", "optim_inactive_first", "optim_inactive_middle", "optim_inactive_last", "optim_n_smallest",
              "optim_n_with_tail_gap", "optim_clip_on", "optim_clip_off", "optim_some_tensor_clips", "optim_some_tensor_does_not_clip",
              "optim_t_total=-1", "optim_two_steps"] + ["optim_shadows_" + s for s in C.OPTIM_SHADOWS] + ["optim_" + s for s in C.SCHEDULES]
             + ["optim_step_" + s for s in C.OPTIM_STEPS] + ["optim_scaler_" + s for s in C.OPTIM_SCALER],
}

DEFECTS = {
    "lmf": ["pad_unmasked", "zs_with_col0", "tie_higher", "label0_counted", "no_rescale", "entries_beyond_256_skipped"],
    "lms": ["tie_higher", "k_largest", "no_1e-5", "hits_zero_weight"],
    "lmb": ["sval_in_col0", "no_smoothing_ge_1024", "dropped_contribute", "repeat_counted_once", "any_pad_unwritten"],
    "lmchain": [],
    "bce": ["infer_may_return_0", "cross_wave_tie_higher", "cols_ge_256_skipped", "unstable_loss"],
    "bceml": ["pos_weight_on_negative", "cols_ge_64_skipped", "pred_at_z>=0"],
    "rmul": ["neg_b_ignored", "cols_ge_256_skipped"],
    "optim": ["gap_in_norm", "tail_not_updated", "decay_unflagged", "clip_squared", "step_off_by_one", "inactive_updated"],
}


def _cases(fam):
    return C.FAMILIES[fam][0]()


def test_every_family_has_its_lists():
    assert set(REQUIRED) == set(DEFECTS) == set(C.FAMILIES)


@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_every_named_branch_is_reached(fam):
    count = C.census(fam)
    print(f"\n{fam}: {len(_cases(fam))} cases")
    for name in sorted(set(REQUIRED[fam]) | set(count)):
        print(f"    {name:40s} {count.get(name, 0):4d}{'' if name in REQUIRED[fam] else '   (not required)'}")
    missing = [n for n in REQUIRED[fam] if not count.get(n)]
    assert not missing, f"{fam}: branches no case reaches: {missing}"


def test_the_value_sets_of_the_sweep_are_all_drawn():
    def seen(fam, *keys):
        return {tuple(c[k] for k in keys) if len(keys) > 1 else c[keys[0]] for c in _cases(fam)}
    three = {C.F32, C.BF16, C.F16}
    # lmf / lmb: every vocabulary, the workload's once per route with at most 8 rows, smoothing only where the ABI has it
    assert seen("lmf", "V") == set(C.LM_V) == seen("lmb", "V")
    assert {c["ls"] for c in C.lmf_cases() if c["V"] >= 3} == set(C.LM_SMOOTH) and {c["ls"] for c in C.lmf_cases() if c["V"] < 3} == {0.0}
    for c in C.lmf_cases():
        assert c["V"] != C.WORKLOAD_V or (c["ld"] == C.WORKLOAD_LD and c["rows"] <= C.WORKLOAD_ROWS), c
    for V in C.LM_V:
        assert {c["ddt"] for c in C.lmb_cases() if c["V"] == V} == three, V                       # each size meets every dtype
        assert {C.lmf_vec(c) for c in C.lmf_cases() if c["V"] == V} == {True, False}, V
        assert {C.lmb_vec(c) for c in C.lmb_cases() if c["V"] == V} == {True, False}, V
    assert {c["ddt"] for c in C.lmb_cases() if "lmb_vec:d_base+8B" in C.lmb_branch(c)} >= {C.BF16}
    # lms
    assert seen("lms", "B") == set(C.LMS_B) and seen("lms", "kname") == set(C.LMS_K)
    assert {(B, k) for B in C.LMS_B for k in C.LMS_K} == seen("lms", "B", "kname")
    # bce
    assert seen("bce", "A") == set(C.BCE_A) and seen("bce", "R") == set(C.BCE_R) and seen("bce", "ddt") == set(C.BCE_DDT)
    for A in C.BCE_A:
        cs = [c for c in C.bce_cases() if c["A"] == A]
        assert {c["ddt"] for c in cs} == set(C.BCE_DDT) and {c["ld"] - A for c in cs} == {0, 1, 6} and {c["ldd"] - A for c in cs} == {0, 6}, A
    assert seen("bce", "absent") == set(C.BCE_ABSENT)
    # bceml
    assert seen("bceml", "C") == set(C.BCEML_C) and seen("bceml", "R") == set(C.BCEML_R) and seen("bceml", "absent") == set(C.BCEML_ABSENT)
    for Cc in C.BCEML_C:
        assert {c["ddt"] for c in C.bceml_cases() if c["C"] == Cc and c["absent"] not in ("dgrad", "target")} == three, Cc
        assert {c["pw"] for c in C.bceml_cases() if c["C"] == Cc} >= {"none", "drawn"}, Cc
    # rmul
    assert seen("rmul", "H", "dt") == {(h, d) for h in C.RMUL_H for d in three} and seen("rmul", "R", "dt") == {(r, d) for r in C.RMUL_R for d in three}
    assert seen("rmul", "neg", "dt") == {(n, d) for n in C.RMUL_NEG for d in three} and seen("rmul", "pad") == {0, 8}
    # optim
    assert {n for c in C.optim_cases() for n in c["counts"]} == set(C.OPTIM_COUNTS)
    assert {len(c["counts"]) for c in C.optim_cases()} == set(range(1, 13))
    assert seen("optim", "mgn") == {-1.0, 1.0} and seen("optim", "sched") == set(C.SCHEDULES) and seen("optim", "t_total") == {-1, 10}
    assert 1 / 10 == 0.1 and C.optim_hyper(dict(where="at"))["warmup"] == 0.1                       # x == warmup exactly at step 1 of 10
    assert all(C.optim_lr(dict(c, where="past"), 10) == 0.0 for c in C.optim_cases() if c["sched"] == "warmup_linear" and c["t_total"] > 0)


def test_the_caps_in_the_sources_are_the_caps_of_the_predicates():
    lm, vqa, opt = (open(os.path.join(CSRC, f)).read() for f in ("mv_lmloss.hip", "mv_vqa.hip", "mv_optim.hip"))
    hdr = open(os.path.join(ROOT, "include", "medvill.h")).read()

    def num(pattern, text):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert num(r"#define\s+MV_OPTIM_CHUNK\s+(\d+)", hdr) == C.OPTIM_CHUNK and "#define CH MV_OPTIM_CHUNK" in opt
    assert C.OPTIM_CHUNK % C.VEC_STRIDE == 0 and num(r"static_assert\(CH % (\d+) == 0", opt) == C.VEC_STRIDE
    assert num(r"const int j = pass \* (\d+) \+ tid \* 4;", opt) == C.VEC_STRIDE
    # 256-thread blocks: every lm kernel, bce_kernel, both chunk kernels; 64-thread blocks: bce_ml_kernel, sq_tensor_kernel
    assert {int(x) for x in re.findall(r"__launch_bounds__\((\d+)\)", lm)} == {C.BLOCK}
    assert len(re.findall(r"block\(%d\)" % C.BLOCK, lm)) == 2 and "dim3(1), dim3(%d), lds" % C.BLOCK in lm
    assert re.findall(r"__launch_bounds__\((\d+)\)", vqa) == [str(C.BLOCK)] * 2 and len(re.findall(r"block\(%d\)" % C.BLOCK, vqa)) == 2
    assert sorted(re.findall(r"__launch_bounds__\((\d+)\)", opt)) == sorted([str(C.BLOCK)] * 2 + [str(C.WAVE)] * 2)
    assert "dim3 grid(R), block(%d);" % C.WAVE in opt and "dim3(NC), dim3(%d)" % C.BLOCK in opt and "dim3(T), dim3(%d)" % C.WAVE in opt
    # the loop strides
    assert len(re.findall(r"c \+= %d\)" % C.VEC_STRIDE, lm)) == 3 and len(re.findall(r"c = tid \* 4; c < \w+; c \+= (\d+)", lm)) == 3
    assert len(re.findall(r"c = tid; c < \w+; c \+= %d\)" % C.BLOCK, lm)) == 3
    assert re.search(r"for \(int e = e0 \+ tid; e < e1; e \+= %d\)" % C.BLOCK, lm)
    assert len(re.findall(r"for \(int b = tid; b < B; b \+= %d\)" % C.BLOCK, lm)) == 2
    assert re.search(r"for \(int c = tid; c < A; c \+= %d\)" % C.BLOCK, vqa) and re.search(r"for \(int c = lane; c < C; c \+= %d\)" % C.WAVE, opt)
    assert re.search(r"for \(int c = lane \* 4; c < H; c \+= %d\)" % C.ROWS_MUL_STRIDE, vqa) and "blockIdx.x * 4 + (threadIdx.x >> 6)" in vqa
    # the selection's cap and its LDS bytes per sample
    assert num(r"if \(B > (\d+)\) return MV_E_SHAPE;", lm) == C.SELECT_MAX_B
    assert "(size_t)B * (2 * sizeof(double) + 2 * sizeof(int))" in lm and 2 * 8 + 2 * 4 == C.SELECT_LDS_PER_SAMPLE
    assert C.SELECT_MAX_B * C.SELECT_LDS_PER_SAMPLE <= 64 * 1024
    # the vector-route conditions the predicates restate
    assert "const bool vec = (ld & 3) == 0 && (((uintptr_t)logits) & 15) == 0;" in lm
    assert "const bool vec = (ld & 3) == 0 && (ldd & 3) == 0 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)dlogits) & dal) == 0;" in lm
    assert "const uintptr_t dal = (uintptr_t)(4 * mv_dtype_size(d_dtype) - 1);" in lm


def test_generated_cases_are_inside_the_abi():
    """A generator that draws what the launcher rejects is a bug in the generator: the GPU file has no way to drop a case."""
    assert C.GUARD % 8 == 0
    for c in C.lmf_cases() + C.lmb_cases() + C.lmchain_cases():                                 # lm_check
        assert c["V"] > 0 and c["ld"] >= c["V"] and 0.0 <= c["ls"] <= 1.0 and (c["ls"] == 0.0 or c["V"] >= 3), c
        assert c["fam"] == "lmf" or c["ldd"] >= c["V"], c
        inp = C.lmf_inputs(c) if c["fam"] == "lmf" else C.lmb_inputs(c)
        assert np.all((inp["labels"] >= 0) & (inp["labels"] < c["V"])) and np.all(np.diff(inp["row_ptr"]) >= 0), c
        assert inp["row_ptr"][0] == 0 and inp["row_ptr"][-1] == inp["labels"].size, c
        if c["fam"] != "lmf":
            assert np.all((inp["sample"] >= 0) & (inp["sample"] < C.LMB_B)), c
    for c in C.lms_cases():
        inp = C.lms_inputs(c)
        assert 0 < c["B"] <= C.SELECT_MAX_B and 0 <= c["k"] <= c["B"], c
        assert inp["w"].size == 0 or (inp["sample"].min() >= 0 and inp["sample"].max() < c["B"]), c
    for c in C.bce_cases():
        assert c["A"] > 0 and c["R"] > 0 and c["ld"] >= c["A"] and c["ldd"] >= c["A"], c
    for c in C.bceml_cases():
        assert c["C"] > 0 and c["R"] > 0 and c["ld"] >= c["C"] and c["ldd"] >= c["C"], c
    for c in C.rmul_cases():                                                                     # every leading dimension a whole number of vectors
        assert c["H"] % 4 == 0 and (c["H"] + c["pad"]) % 4 == 0 and c["R"] > 0, c
        inp = C.rmul_inputs(c)
        assert inp["ra"].max() < inp["a"].shape[0] and inp["rb"].max() < inp["b"].shape[0], c
    for c in C.optim_cases():                                                                    # the table invariants of mv_optim.hip
        ent, n = C.optim_layout(c)
        tensors, chunks = C.optim_tables(ent)
        assert n % 4 == 0 and n >= ent[-1][0] + ent[-1][1] and 1 <= len(ent) <= 12, c
        end = 0
        for t, (off, cnt, first, flags) in enumerate(tensors.tolist()):
            nch = (cnt + C.OPTIM_CHUNK - 1) // C.OPTIM_CHUNK
            assert off % 64 == 0 and off >= end and cnt > 0 and chunks[first:first + nch].tolist() == [t] * nch, (c, t)
            end = off + cnt
        assert len(chunks) == sum((e[1] + C.OPTIM_CHUNK - 1) // C.OPTIM_CHUNK for e in ent)
        assert c["tail"] or n == (end + 3) // 4 * 4, c                                           # the smallest legal n
    for fam in C.FAMILIES:                                                                       # a printed cfg reproduces the case
        seeds = [c["seed"] for c in _cases(fam)]
        assert len(set(seeds)) == len(seeds), fam
    a, b = C.lmf_inputs(C.lmf_case(5)), C.lmf_inputs(dict(C.lmf_case(5)))
    assert np.array_equal(a["logits"].view(np.int32), b["logits"].view(np.int32)) and np.array_equal(a["labels"], b["labels"])


def test_the_gpu_file_cannot_drop_a_case():
    src = open(GPU_FILE).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break, ast.Try)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            assert "unittest" not in ast.dump(node), f"line {node.lineno}"
    for fam, (cases, _) in C.FAMILIES.items():              # one parametrised test per family over its full case list
        assert re.search(r'parametrize\("cfg", C\.%s\(\)' % cases.__name__, src), cases.__name__
    assert "pytestmark = pytest.mark.gpu" in src


def test_the_generators_meet_their_conditions():
    """lms: sums that are not exactly tied differ by 1e-9 of the largest, so the kernel's double sums (error about n 2^-53) cannot
    reorder them; exact ties are copies (same entries, same order) or sums that are exactly zero in any arithmetic.  lmchain: the
    sample sums lie far enough apart for the f32 entry losses of the forward kernel."""
    for c in C.lms_cases():
        inp = C.lms_inputs(c)
        L, _, _ = C.lms_sums(inp, c["B"])
        s = np.sort(np.array(L))
        gaps = np.diff(s)
        assert np.all((gaps == 0) | (gaps >= C.LMS_GAP * max(s.max(), 1e-300))), c
        tied = {}
        for b, v in enumerate(L):
            tied.setdefault(v, []).append(b)
        for v, bs in tied.items():
            if len(bs) > 1 and v != 0.0:
                ent = {tuple((float(inp["loss"][e]), float(inp["w"][e])) for e in range(inp["w"].size) if inp["sample"][e] == b) for b in bs}
                assert len(ent) == 1, (c, bs)
        for a, b in inp["copies"]:
            assert L[a] == L[b]
    for c in C.lmchain_cases():
        ref = C.lmchain_reference(c, C.lmchain_inputs(c))
        s = np.sort(np.array(ref["sums"]))
        assert np.all(s >= 0) and np.all((np.diff(s) == 0) | (np.diff(s) > 1e-3 * s[1:])), (c, s)         # (the entry losses carry about 1e-6)
        assert 0 < ref["keep"].sum() == C.LMCHAIN_K


def test_the_references_state_what_they_are_meant_to():
    """the per-label closed form against the target-row form of report_finetune_cases.slot_loss, fp64 against fp64"""
    for i in (2, 3, 4, 17, 20, 31):
        c = C.lmf_case(i)
        inp = C.lmf_inputs(c)
        for u in range(c["rows"]):
            lab = inp["labels"][inp["row_ptr"][u]:inp["row_ptr"][u + 1]][:5].astype(np.int64)
            z = inp["logits"][u, :c["V"]]
            if lab.size == 0 or not np.all(np.isfinite(z)):
                continue
            mine = C.lm_row_loss(z, lab, c["ls"])[0]
            zz = torch.from_numpy(z.astype(np.float64)).expand(lab.size, -1)
            theirs = RF.slot_loss(zz, torch.from_numpy(lab), c["ls"]).numpy()
            assert np.max(np.abs(mine - theirs)) < 1e-10 * (1 + np.max(np.abs(theirs))), (c, u)
    assert RF.smoothing_constants(0.1, 30522)[1] == C.lm_const(0.1, 30522)[2]
    # the backward's reference is the derivative of the forward's objective (exact constants up to their f32 rounding)
    c = dict(C.lmb_case(3), ls=0.1, ddt=C.F32)
    inp = C.lmb_inputs(c)
    ref = C.lmb_reference(c, inp)
    V, u = c["V"], C.LMB_ROWS.index("mixed")
    z = torch.from_numpy(inp["logits"][u, :V].astype(np.float64)).requires_grad_(True)
    e0, e1 = inp["row_ptr"][u], inp["row_ptr"][u + 1]
    lab = torch.from_numpy(inp["labels"][e0:e1].astype(np.int64))
    cf = torch.tensor([float(inp["w"][e]) * int(inp["keep"][inp["sample"][e]]) for e in range(e0, e1)], dtype=torch.float64)
    (RF.slot_loss(z.expand(lab.numel(), -1), lab, 0.1) * cf).sum().backward()
    G = float(inp["g"]) * (inp["lsv"] or 1.0) * float(inp["inv"][0])
    assert float((z.grad * G - torch.from_numpy(ref["grad"][u])).abs().max()) < 1e-6 * G
    # half an ulp of the 16-bit encodings, against the encodings themselves
    x = torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.9921875, 3.0, 0.3125], dtype=torch.float64)
    for enc in (C.BF16, C.F16):
        nxt = (x.to(C.DT[enc]).view(torch.int16) + 1).view(C.DT[enc]).double()
        assert bool(((nxt - x) / 2 <= C.HALF_ULP_REL[enc] * x).all())


@pytest.mark.parametrize("fam", sorted(C.FAMILIES))
def test_an_honest_f32_restatement_passes_every_case(fam):
    worst = 0.0
    for cfg in _cases(fam):
        ok, ratio, what = C.run_restated(cfg)
        assert ok, (what, cfg)
        worst = max(worst, ratio)
    print(f"\n{fam}: honest restatement over {len(_cases(fam))} cases, worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fam,defect", [(f, d) for f in sorted(DEFECTS) for d in DEFECTS[f]])
def test_each_planted_defect_fails_some_case(fam, defect):
    caught = [(c, C.run_restated(c, defect)[2]) for c in _cases(fam)]
    caught = [(c, w) for c, w in caught if w]
    print(f"\n{fam} / {defect}: caught by {len(caught)} of {len(_cases(fam))} cases" + (f", e.g. {C.case_id(caught[0][0])}: {caught[0][1][:160]}" if caught else ""))
    assert caught, (fam, defect)


def test_spot_check_smoothing_dropped_beyond_the_first_trip():
    """The smoothing term dropped for columns >= 1024 fails a case with V >= 2049 in every output dtype under the derived bounds; under
    the largest-absolute-error tolerance of the hand-picked tests it passes in bf16 (DESIGN.md has the figures)."""
    failed, old = set(), {}
    for c in C.lmb_cases():
        if c["V"] < 2049 or c["ls"] == 0:
            continue
        inp = C.lmb_inputs(c)
        ref = C.lmb_reference(c, inp)
        out = C.lmb_restated(c, inp, "no_smoothing_ge_1024")
        ok, ratio, _ = C.lmb_judge(c, inp, ref, out)
        passes, err = C.old_scheme_passes(c, inp, ref, out)
        print(f"{C.case_id(c)}: error / bound {ratio:.3g}; largest absolute error {err:.3g} -> the old tolerance {'passes' if passes else 'fails'}")
        if not ok:
            failed.add(c["ddt"])
        old.setdefault(c["ddt"], []).append(passes)
    assert failed == {C.F32, C.BF16, C.F16}
    assert all(old[C.BF16])


def test_spot_check_the_second_trip_of_the_multilabel_loop():
    caught = {c["C"] for c in C.bceml_cases() if not C.run_restated(c, "cols_ge_64_skipped")[0]}
    missed = {c["C"] for c in C.bceml_cases() if C.run_restated(c, "cols_ge_64_skipped")[0]}
    assert caught == {65, 130} and missed == set(C.BCEML_C) - {65, 130}


def test_inputs_carry_what_the_checks_need():
    for c in C.lmf_cases():
        inp = C.lmf_inputs(c)
        assert np.all(inp["logits"][:, c["V"]:] == np.float32(1e30)), c                         # every pad column
        for u, p in enumerate(inp["patterns"]):
            z = inp["logits"][u, :c["V"]]
            if p.startswith("dup_"):
                assert (z == z.max()).sum() == 2, (c, u)
            if p == "asc":
                assert np.all(np.diff(z) > 0), c
            if p == "desc":
                assert np.all(np.diff(z) < 0), c
            if p == "asc" and c["V"] >= 1024:
                assert C.lm_thread_rises(z, C.lmf_vec(c)) >= c["V"] // C.BLOCK, c               # the running maximum rises again and again
    for c in C.bceml_cases():
        if c["pattern"] == "edges":
            z, y = C.bceml_inputs(c)["calls"][0]
            assert np.any(z[:, :c["C"]] == 0) and np.any(y == 0.5), c
    for c in C.lmb_cases():
        inp = C.lmb_inputs(c)
        dead = [u for u, w in enumerate(inp["dead"]) if w]
        assert len(dead) >= 3 and np.all(np.isnan(inp["logits"][dead])), c
    for c in C.optim_cases():
        inp, (ent, n) = C.optim_inputs(c), C.optim_layout(c)
        mask = np.zeros(n, bool)
        for off, cnt, _, _ in ent:
            mask[off:off + cnt] = True
        assert np.all(inp["g"][~mask] == np.float32(1e3)) and np.all(inp["p"][~mask] == np.float32(C.SENT["p"])), c
        assert math.isfinite(C.optim_lr(c, 1))
