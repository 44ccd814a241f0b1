"""n-gram blocking, CPU side: the plain-Python rule of tests/ngram_cases.py against traces recorded from the reference's own beam
search (tests/golden/ngram_beam.npz, written by tools/gen_ngram_golden.py), the branch census of the kernel sweep, the limits in the
source and the header, planted defects, the ABI bookkeeping and generate()'s argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import decode_cases as D
import ngram_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc", "mv_decode.hip")
HEADER = os.path.join(ROOT, "include", "medvill.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ngram_beam.npz")
MIN_HITS = 3

REQUIRED = {
    "nb": ["n=%d" % n for n in range(C.NB_MIN_N, C.NB_MAX_N + 1)] + ["L=%d" % v for v in C.NB_L]
          + ["L<n", "L==n", "L>n", "L==n-1", "L==n+1", "no_match", "one_match", "several_matches", "dedup", "several_words", "found_out_of_order",
             "window_overlaps_tail", "last_window_only", "ignore_in_tail", "ignore_in_tail_hides_a_ban", "ignore_candidate", "ignore_none",
             "ignore_some", "ignore_cap", "parent_null", "parent_perm", "parent_shared", "many_rows_one_parent", "ld_h>L", "ld_ban>need",
             "more_windows_than_threads"],
    "tkb": ["km1", "km4", "km16", "k==V"] + list(C.TKB_MODES)
           + ["banned_column_emitted", "selection_changed_by_ban", "id_out_of_range", "id_listed_twice", "eos_banned_and_penalised",
              "best_column_banned", "more_bans_than_a_list_holds", "ld_ban>nban", "penalised_values_collide"],
}


# ---- the rule against the reference's own traces -------------------------------------------------------------------------------
def _golden_cases():
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    return z, names


def test_restatement_reproduces_every_reference_trace():
    z, names = _golden_cases()
    assert len(names) >= 8
    seen = set()
    for name in names:
        g = lambda k: z[f"{name}/{k}"]
        B, K, n, eos, min_len, steps = (int(g(k)) for k in ("B", "K", "n", "eos_id", "min_len", "steps"))
        lp_pen = float(g("length_penalty"))
        ignore = g("ignore").tolist()
        tables = [torch.log_softmax(torch.from_numpy(t), dim=-1) for t in g("tables")]
        rec = []
        ids, best, tr = C.blocked_beam(tables, B, K, eos, min_len, lp_pen, steps, n, ignore or None, record=rec)
        assert torch.equal(tr["pred_seq"], torch.from_numpy(g("pred_seq"))[:, :steps]), name
        assert torch.equal(tr["wids"], torch.from_numpy(g("wids"))[:, :steps]), name
        assert torch.equal(tr["ptrs"], torch.from_numpy(g("ptrs"))[:, :steps]), name
        assert torch.allclose(tr["scores"], torch.from_numpy(g("scores"))[:, :steps], atol=1e-5), name
        # what the issue asks the fixture to hold
        _, _, off = C.blocked_beam(tables, B, K, eos, min_len, lp_pen, steps, 0)
        assert not torch.equal(off["wids"], tr["wids"]), name
        seen |= {"K=%d" % K, "n=%d" % n}
        seen |= {"ignore"} if ignore else {"no_ignore"}
        seen |= {"min_len"} if min_len else set()
        seen |= {"length_penalty"} if lp_pen else set()
        w = tr["wids"]
        if min_len and any(eos in C.banned_words(s, n, ignore) for fr in rec[:min_len - 1] for s in fr):
            seen.add("eos_banned_while_min_len_holds")
        if any(eos in s[:-1] for s in rec[-1]):
            seen.add("beam_extends_after_eos")
    want = {"K=1", "K=3", "K=4", "n=2", "n=3", "n=4", "ignore", "no_ignore", "min_len", "length_penalty", "eos_banned_while_min_len_holds",
            "beam_extends_after_eos"}
    assert want <= seen, want - seen


# ---- census --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_every_named_branch_is_reached(fam):
    count = C.census(fam)
    print(f"\n{fam}: {len(C.FAMILIES[fam][0]())} cases")
    for name in sorted(set(REQUIRED[fam]) | set(count)):
        print(f"    {name:48s} {count.get(name, 0):4d}{'' if name in REQUIRED[fam] else '   (not required)'}")
    short = {n: count.get(n, 0) for n in REQUIRED[fam] if count.get(n, 0) < MIN_HITS}
    assert not short, f"{fam}: branches reached fewer than {MIN_HITS} times: {short}"


def test_generated_cases_are_inside_the_abi():
    for c in C.nb_cases():
        assert C.NB_MIN_N <= c["n"] <= C.NB_MAX_N and 1 <= c["L"] <= C.NB_MAX_LEN and c["ld_h"] >= c["L"] and c["n_ign"] <= C.NB_MAX_IGN, c
        assert c["ld_ban"] >= c["L"] + 1 - c["n"] and c["ld_ban"] >= 1, c
        i = C.nb_inputs(c)
        assert i["parent"] is None or (0 <= int(i["parent"].min()) and int(i["parent"].max()) < c["R"]), c
        assert all(len(s) == c["L"] for s in i["seqs"]) and all(len(b) <= c["ld_ban"] for b in C.nb_expected(c, i)), c
        assert bool((i["hist_in"][:, c["L"] - 1:] == C.HIST_SENTINEL).all()), c
    for c in C.tkb_cases():
        assert 0 < c["k"] <= min(D.TK_MAX_K, c["V"]) and c["V"] <= C.TKB_MAX_V and c["ld_ban"] >= 1, c
        x, ban, nban = C.tkb_inputs(c)
        assert (ban is None) == (c["ban_mode"] == "ban_null") and (ban is None or int(nban.max()) <= c["ld_ban"]), c


def test_topk_order_is_decided_for_all_but_a_small_share_and_empty_bans_change_nothing():
    """The f64 reference alone: at most 2 % of the emitted entries sit closer to a neighbour than the bounds can tell apart; with no
    ban the reference is decode_cases.tk_reference."""
    emitted = excused = 0
    for c in C.tkb_cases():
        x, ban, nban = C.tkb_inputs(c)
        x64 = x[:, :c["V"]].double()
        eos = D.tk_eos(c)
        ref = C.tkb_reference(x64, c["k"], eos, ban, nban)
        ex = C.tkb_excused(ref, C.tkb_bound(ref, D.TK_TOL))
        emitted += ex.numel()
        excused += int(ex.sum())
        if c["ban_mode"] in ("ban_null", "ban_empty"):
            v, i, l = D.tk_reference(x64, c["k"], eos)
            assert torch.equal(ref["idx"], i) and torch.equal(ref["vals"], v) and torch.equal(ref["lse"], l), c
        if 0 <= eos < c["V"]:
            assert bool((ref["vals"][ref["idx"] == eos] == C.BAN_PENALTY).all()), c
    print(f"\ntkb: {excused} of {emitted} emitted entries excused")
    assert excused <= 0.02 * emitted, (excused, emitted)


def test_the_gpu_file_cannot_drop_a_case():
    import ast
    src = open(os.path.join(ROOT, "tests", "test_ngram_sweep_gpu.py")).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
    for cases in ("nb_cases", "tkb_cases"):
        assert re.search(r'parametrize\("cfg", C\.%s\(\)' % cases, src), cases


# ---- limits in the source and the header ---------------------------------------------------------------------------------------
def test_the_limits_in_the_source_and_the_header_agree_with_the_case_module():
    src = open(HIP).read()
    hdr = re.sub(r"\s+\*\s+", " ", open(HEADER).read())

    def num(pattern, text=src):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert num(r"#define NB_MAX_LEN (\d+)") == C.NB_MAX_LEN and num(r"#define NB_MAX_IGN (\d+)") == C.NB_MAX_IGN
    assert num(r"#define NB_MIN_N (\d+)") == C.NB_MIN_N and num(r"#define NB_MAX_N (\d+)") == C.NB_MAX_N
    assert num(r"#define TKB_MAX_V (\d+)") == C.TKB_MAX_V
    assert num(r"for \(int i = tid; i < W; i \+= (\d+)\)") == C.NB_THREADS
    assert "lp + -10000.0f" in src and C.BAN_PENALTY == D.TK_EOS_LOGPROB
    assert (num(r"(\d+) <= n <= \d+ \(MV_E_ARG\)", hdr), num(r"\d+ <= n <= (\d+) \(MV_E_ARG\)", hdr)) == (C.NB_MIN_N, C.NB_MAX_N)
    assert num(r"len \+ 1 <= (\d+),", hdr) == C.NB_MAX_LEN and num(r"n_ign <= (\d+),", hdr) == C.NB_MAX_IGN
    assert num(r"V <= (\d+) \(one LDS bit per column", hdr) == C.TKB_MAX_V
    from medvill_amd import generate as G
    assert (G.NGRAM_MIN, G.NGRAM_MAX, G.NGRAM_MAX_IGNORE, G.NGRAM_MAX_LEN) == (C.NB_MIN_N, C.NB_MAX_N, C.NB_MAX_IGN, C.NB_MAX_LEN)
    assert C.PENALTY_HALF_ULP == float(np.spacing(np.float32(10000.0))) / 2


# ---- planted defects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,branch", [("no_dedup", "dedup"), ("no_ignore_tail", "ignore_in_tail_hides_a_ban"),
                                           ("short_last_window", "last_window_only")])
def test_a_planted_defect_in_the_rule_changes_the_ban_lists(defect, branch):
    hit = 0
    for c in C.nb_cases():
        if branch in C.nb_branches(c):
            i = C.nb_inputs(c)
            assert C.nb_expected(c, i, defect) != C.nb_expected(c, i), (defect, c)
            hit += 1
    assert hit >= MIN_HITS


@pytest.mark.parametrize("defect", ["before_normalisation", "fill"])
def test_a_planted_defect_in_the_penalty_lands_outside_the_bounds(defect):
    hit = 0
    for c in C.tkb_cases():
        if "banned_column_emitted" not in C.tkb_branches(c) and not (defect == "before_normalisation" and "best_column_banned" in C.tkb_branches(c)):
            continue
        x, ban, nban = C.tkb_inputs(c)
        x64 = x[:, :c["V"]].double()
        eos = D.tk_eos(c)
        ref = C.tkb_reference(x64, c["k"], eos, ban, nban)
        bad = C.tkb_reference(x64, c["k"], eos, ban, nban, defect=defect)
        lp_cpu, _ = D.tk_f32_cpu(x[:, :c["V"]], c["k"], eos)
        tol = D.case_tol(D.TK_TOL, lp_cpu.gather(1, D.tk_reference(x64, c["k"], eos)[1]), D.tk_reference(x64, c["k"], eos)[0])
        bound = C.tkb_bound(ref, tol)
        fin = torch.isfinite(ref["vals"]) & torch.isfinite(bad["vals"])
        off = (not torch.equal(bad["idx"], ref["idx"])) or bool(((bad["vals"] - ref["vals"]).abs()[fin] > bound[fin]).any())
        moved = ref["banned"] & fin & ((ref["vals"] - C.BAN_PENALTY).abs() > bound)
        if defect == "fill" and bool(moved.any()):
            assert off, c                 # a filled penalty moves every emitted banned value by its log-prob
        hit += int(off)
    assert hit >= MIN_HITS, hit


# ---- ABI bookkeeping and generate()'s argument checks ----------------------------------------------------------------------------
def test_new_abi_symbols_are_declared_and_exported():
    import medvill_amd  # noqa: F401
    from medvill_amd import _lib
    from tests.test_abi import header_functions
    decl = header_functions()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in (("mv_ngram_ban", 14), ("mv_logprob_topk_banned", 13)):
        assert decl.get(name) == n and len(_lib.PROTOTYPES[name]) == n
        assert hasattr(raw, name)
    assert decl["mv_logprob_topk"] == 10                      # the unbanned entry keeps its signature
    assert _lib.load().mv_abi_version() == 6


def test_generate_argument_checks():
    from medvill_amd.generate import generate

    class Fake:
        pass
    for kw in (dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=3, forced_ids=torch.zeros((1, 4), dtype=torch.int64)),
               dict(no_repeat_ngram_size=2, no_repeat_ignore_ids=range(C.NB_MAX_IGN + 1))):
        with pytest.raises(ValueError):
            generate(Fake(), None, None, None, **kw)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        generate(Fake(), None, None, None, forbid_duplicate_ngrams=True)
    with pytest.raises(NotImplementedError, match="no_repeat_ignore_ids"):
        generate(Fake(), None, None, None, forbid_ignore_set={5})
