"""Branch census and defect check of the sweep of the batch-assembly and row-plan kernels (CPU).  tests/test_batch_sweep_gpu.py is only
worth its GPU time while its cases reach every branch of csrc/mv_batch.hip and its judgement can tell a right kernel from a wrong
one; this file counts the branches, reads the constants the restatements rely on out of the sources and the header, runs the numpy
restatement of every kernel -- and the same restatement with one defect planted at a time -- through the very references and
judgement the GPU file applies, checks the draw stream's statistics on the numpy hash (the GPU file then needs equality only),
compares the references with the project's host twins, and exercises every argument reject of the four entry points."""
import ast
import math
import os
import re

import numpy as np
import pytest
import torch

import batch_cases as C
import rowops_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc")
GPU_FILE = os.path.join(ROOT, "tests", "test_batch_sweep_gpu.py")

REQUIRED = {
    "draws": ["n=1", "n=255", "n=256", "n=257", "n=773", "blocks=1", "blocks>1", "last_block_full", "last_block_partial", "key_hi=0", "key_hi!=0",
              "pair_2B", "pair_SB", "B>1_and_S>1"] + ["vocab=%d" % v for v in C.DRAW_VOCABS],
    "corrupt": ["L=%d" % v for v in C.CORRUPT_L] + ["N=%d" % v for v in C.CORRUPT_N] + ["B=%d" % v for v in C.CORRUPT_B]
               + ["draws_" + d for d in C.CORRUPT_DRAWS]
               + ["trips=1", "trips=2", "trips=3", "n2<256", "n2==256", "n2>256", "counts_loop_second_trip", "second_trip_adds_a_count",
                  "len<0", "len=0", "len=1", "len=S-1", "len=S", "len>S", "zero_length_first", "zero_length_middle", "zero_length_last",
                  "zero_count_inside_the_prefix_sum", "len0_no_forced_mask", "forced_mask", "forced_label_in_thread_0's_own_element",
                  "forced_label_in_another_thread's_element", "every_token_selected", "index_exactly_full", "index_empty",
                  "only_the_last_token_selected", "labels_at_lanes_0_63_and_threads_0_255", "full_wave_of_labels",
                  "labels_behind_a_full_wave_in_its_trip", "labels_in_several_trips", "labels_in_several_waves_of_a_trip",
                  "act_mask", "act_random", "act_keep", "act_none", "rnd=0_used", "rnd=102_used", "rnd=103_used",
                  "every_edge_draw_on_a_valid_token", "family_given", "family_null", "desc_given", "desc_null", "index_given", "index_null"],
    "pack": ["B=%d" % v for v in C.PACK_B] + ["L=%d" % v for v in C.PACK_L]
            + ["vl<0", "vl=0", "vl=1", "vl=L-1", "vl=L", "vl>L", "classes_mixed_in_a_batch", "cu[B]=0", "cu[B]=B*L", "cu[B]_between",
               "prefix_trips=0", "prefix_trips=1", "prefix_trips=2", "second_trip_adds_a_count", "row_trips=1", "row_trips=2", "row_trips=3",
               "last_sample_drops_positions"],
    "tail": ["rows=%d" % v for v in (0, 1, 63, 64, 65, 256, 257, 2048)] + ["B=1", "B=5", "B=300", "L=2048"]
            + ["n_sel=%s" % v for v in C.TAIL_NSEL] + ["n_sel>cu[B]", "sel_trips=1", "sel_trips=2", "cu[B]=0", "sel_shuffled", "sel_duplicates",
               "sel_minus1", "sel_below_minus1", "sel_beyond_cu[B]", "sel_equals_cu[B]", "sample_with_no_selected_row",
               "sample_with_every_row_selected", "sample_partly_selected", "sel_offset_0", "sel_offset_63", "sel_offset_64", "sel_offset_n-1",
               "partition_over_several_chunks"],
    "chain": ["shape=%dx%dx%d" % s for s in C.CHAIN_SHAPES] + ["family_full", "family_1d", "len=1", "len=S", "sample_without_natural_selection",
              "extra_none", "extra_dropped", "sel_names_a_dropped_position", "sel_new=-1", "positions_dropped"],
}

# defect -> the branch names whose cases must ALL reject it (None: every case of the family)
CAUGHT_BY = {
    ("draws", "rnd_mod"): ["vocab=30522", "vocab=%d" % (2 ** 31 - 1)],
    ("draws", "u_low24"): None,
    ("draws", "index_transposed"): ["B>1_and_S>1"],
    ("corrupt", "le_0.15"): ["every_edge_draw_on_a_valid_token"],
    ("corrupt", "le_0.8"): ["every_edge_draw_on_a_valid_token"],
    ("corrupt", "forced_when_len0"): ["len0_no_forced_mask"],
    ("corrupt", "forced_labels_corrupted"): ["forced_mask"],
    ("corrupt", "sep_late"): None,
    ("corrupt", "label_offset_N+1"): ["act_mask", "act_random", "act_keep"],            # (a forced label is stored at N+2 by thread 0 itself)
    ("corrupt", "index_ignores_waves"): ["labels_in_several_waves_of_a_trip"],
    ("corrupt", "index_first_256_counts"): ["second_trip_adds_a_count"],
    ("pack", "no_clamp"): ["vl<0", "vl>L"],
    ("pack", "rowmap_for_dropped"): ["last_sample_drops_positions"],
    ("tail", "unselected_first"): ["sample_partly_selected"],
    ("tail", "qlim_counts_duplicates"): ["sel_duplicates"],
    ("tail", "sel_new_unwritten"): ["sel_minus1", "sel_below_minus1", "sel_beyond_cu[B]"],
    ("chain", "sel_new_unwritten"): ["sel_names_a_dropped_position"],
}


def _cases(fam):
    return C.FAMILIES[fam][0]()


def _branch(cfg):
    return C.branches(cfg)


def test_every_family_has_its_lists():
    assert set(REQUIRED) == set(C.DEFECTS) == set(C.FAMILIES)
    assert {k for k in CAUGHT_BY} == {(f, d) for f, ds in C.DEFECTS.items() for d in ds}
    for fam in C.FAMILIES:                                                                       # a printed cfg reproduces the case
        seeds = [c["seed"] for c in _cases(fam)]
        assert len(set(seeds)) == len(seeds) and all(c["fam"] == fam for c in _cases(fam)), fam
        assert len({C.case_id(c) for c in _cases(fam)}) == len(seeds), fam


# ---- census ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_every_named_branch_is_reached(fam):
    count = C.census(fam)
    print(f"\n{fam}: {len(_cases(fam))} cases")
    for name in sorted(set(REQUIRED[fam]) | set(count)):
        print(f"    {name:48s} {count.get(name, 0):4d}{'' if name in REQUIRED[fam] else '   (not required)'}")
    missing = [n for n in REQUIRED[fam] if not count.get(n)]
    assert not missing, f"{fam}: branches no case reaches: {missing}"


def test_the_census_notices_a_name_that_loses_its_last_case():
    """for every required name that rests on a single case: the census taken without that case reports the name as missing"""
    for fam in sorted(REQUIRED):
        full = C.census(fam)
        last = {}
        for k, c in enumerate(_cases(fam)):
            for name in set(_branch(c)):
                if full[name] == 1 and name in REQUIRED[fam]:
                    last.setdefault(k, []).append(name)
        for k, names in last.items():
            short = C.census(fam, drop=k)
            assert all(not short.get(n) for n in names) and all(short.get(n) for n in REQUIRED[fam] if n not in names), (fam, k)
        print(f"{fam}: {sum(len(v) for v in last.values())} of {len(REQUIRED[fam])} required names rest on a single case")


def test_the_case_lists_hold_the_sizes_the_kernels_branch_on():
    seen = lambda fam, k: {c[k] for c in _cases(fam)}                                               # noqa: E731
    assert {c["B"] * c["S"] for c in C.draws_cases()} >= {1, 255, 256, 257, 3 * 256 + 5} and seen("draws", "vocab") == set(C.DRAW_VOCABS)
    assert {c["S"] + c["N"] + 3 for c in C.corrupt_cases()} == set(C.CORRUPT_L) and seen("corrupt", "N") == set(C.CORRUPT_N)
    assert seen("corrupt", "B") == set(C.CORRUPT_B) and seen("corrupt", "draws") == set(C.CORRUPT_DRAWS)
    assert seen("pack", "B") >= set(C.PACK_B) and seen("pack", "L") >= set(C.PACK_L)
    assert seen("tail", "n_sel") == set(C.TAIL_NSEL) and seen("tail", "sel") == set(C.TAIL_SEL) and seen("tail", "rows") == set(C.TAIL_ROWS)
    assert {(c["B"], c["N"], c["S"]) for c in C.chain_cases()} == set(C.CHAIN_SHAPES)
    for c in C.corrupt_cases():                                                                  # inside the ABI
        assert c["B"] > 0 and c["N"] >= 0 and c["S"] > 0 and c["B"] <= 300, c
    for c in C.pack_cases():
        assert 0 < c["B"] <= 300 and 0 < c["L"] <= 2048, c
    for c in C.tail_cases():
        i = C.tail_inputs(c)
        assert 0 < i["B"] <= 300 and int(np.diff(i["cu"]).max()) <= c["L"] <= C.TP_MAXL and i["n_sel"] > 0 and i["sel"].size == i["n_sel"], c
        assert i["cu"][0] == 0 and (np.diff(i["cu"]) >= 0).all(), c
    a, b = C.corrupt_inputs(C.corrupt_cases()[7]), C.corrupt_inputs(dict(C.corrupt_cases()[7]))
    assert all(np.array_equal(a[k], b[k]) for k in ("ids", "lengths", "u", "rnd", "family"))
    assert C.SENTINEL not in (-1, C.IGNORE) and C.SENTINEL < 0 and C.GUARD % 8 == 0


def test_the_gpu_file_cannot_drop_a_case():
    src = open(GPU_FILE).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break, ast.Try)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
    for fam, entry in C.FAMILIES.items():                    # one parametrised test per family over its full case list
        assert re.search(r'parametrize\("cfg", C\.%s\(\)' % entry[0].__name__, src), fam
    assert "pytestmark = pytest.mark.gpu" in src


# ---- constants -------------------------------------------------------------------------------------------------------------------
def test_the_constants_in_the_sources_and_the_header_are_the_module_s():
    src = open(os.path.join(CSRC, "mv_batch.hip")).read()
    common = open(os.path.join(CSRC, "mv_common.h")).read()
    hdr = re.sub(r"\s*\n\s*\*\s+", " ", open(os.path.join(ROOT, "include", "medvill.h")).read())

    def nums(pattern, text):
        m = re.search(pattern, text)
        assert m, pattern
        return tuple(int(g, 0) for g in m.groups())
    assert nums(r"constexpr int TOK_PAD = (\d+), TOK_SEP = (\d+), TOK_MASK = (\d+);", src) == (C.TOK_PAD, C.TOK_SEP, C.TOK_MASK)
    assert nums(r"constexpr int NT = (\d+);", src) == (C.NT,) and nums(r"#define TP_MAXL (\d+)", src) == (C.TP_MAXL,)
    assert src.count("__launch_bounds__(NT)") == 4 and src.count("<<<B, NT, 0, stream>>>") == 4 and "<<<(n + 255) / 256, 256, 0, stream>>>" in src
    assert C.NT == 4 * C.WAVE and "threadIdx.x & 63" in src and "threadIdx.x >> 6" in src and "c += 64" in src
    m = re.search(r"if \(!\(p < ([\d.]+)\)\) return 0;\s*p /= ([\d.]+);\s*return p < ([\d.]+) \? 1 : \(p < ([\d.]+) \? 2 : 3\);", src)
    assert m and tuple(float(g) for g in m.groups()) == (C.P_SELECT, C.P_SELECT, C.P_MASK, C.P_RANDOM)
    assert "(float)(h0 >> 8) * (1.0f / 16777216.0f)" in src and "(unsigned long long)h1 * (unsigned long long)vocab) >> 32" in src
    assert "mv_hash32(2u * (unsigned)i, k0, k1)" in src and "mv_hash32(2u * (unsigned)i + 1u, k0, k1)" in src
    assert "(unsigned)(key & 0xffffffffULL), (unsigned)(key >> 32)" in src
    assert "if (L > TP_MAXL) return MV_E_SHAPE;" in src and src.count("> 0x7fffffffLL) return MV_E_SHAPE;") == 3
    # the hash
    body = re.search(r"unsigned mv_hash32\(unsigned x, unsigned k0, unsigned k1\) \{(.*?)\n\}", common, re.S).group(1)
    assert tuple(int(v, 16) for v in re.findall(r"\* (0x[0-9A-Fa-f]+)u;", body)) == C.HASH_MUL == R.HASH_MUL
    assert tuple(int(v) for v in re.findall(r"x \^= x >> (\d+);", body)) == C.HASH_SHIFT == R.HASH_SHIFT
    assert re.sub(r"\s*//[^\n]*", "", body).split() == ("x = (x ^ k0) * 0x9E3779B1u; x ^= x >> 15; x = (x ^ k1) * 0x85EBCA6Bu; x ^= x >> 13; "
                                                        "x ^= x >> 16; return x;").split()
    # the buffer sizes the header states, against the module's buffers at one shape
    for text in ("u   f32   [B,S]", "rnd int32 [B,S]", "input_txt  int64 [B,T]  T = S+1", "segment    int64 [B,T]", "txt_labels int64 [B,L]  L = S+N+3",
                 "n_ids      int32 [B]", "desc       int32 [B,3]", "counts     int32 [B]", "label_rows / label_ids int32 [>= B*S], n_labels int32 [1]",
                 "cu     int32 [B+1]", "rowmap int32 [>= cu[B]] (capacity B*L)", "inv    int32 [B*L]", "perm    int32 [cu[B]]", "newpos  int32 [cu[B]]",
                 "qlim    int32 [B]", "sel_new int32 [n_sel]", "<= 2048", "-1 for an entry that lies in no sample", "B*S <= 2^31-1",
                 "out-of-range is clamped to 0..S", "[SEP]=102", "[MASK]=103", "[PAD]=0"):
        assert text in hdr, text
    B, N, S = 7, 36, 217
    T, L = S + 1, S + N + 3
    cfg = dict(B=B, N=N, S=S, pair="none", L=L)
    i32, i64, f32 = C.I32, C.I64, C.F32
    assert C.draws_buffers(cfg) == dict(u=(f32, B * S), rnd=(i32, B * S))
    assert C.corrupt_buffers(cfg) == dict(input_txt=(i64, B * T), segment=(i64, B * T), txt_labels=(i64, B * L), n_ids=(i32, B), desc=(i32, 3 * B),
                                          counts=(i32, B), label_rows=(i32, B * S), label_ids=(i32, B * S), n_labels=(i32, 1))
    assert C.pack_buffers(cfg) == dict(cu=(i32, B + 1), rowmap=(i32, B * L), inv=(i32, B * L))
    ti = dict(B=B, M=100, n_sel=9)
    assert C.tail_buffers(cfg, ti) == dict(perm=(i32, 100 + C.TAIL_SLACK), newpos=(i32, 100 + C.TAIL_SLACK), qlim=(i32, B), sel_new=(i32, 9))
    from medvill_amd import data
    assert data.FAMILY_ID == C.FAMILY_ID and (data.SEP, data.MASK) == (C.TOK_SEP, C.TOK_MASK)


def test_the_shared_hash_is_the_one_hash():
    """rowops_cases.hash32 on scalars written out by hand (Python integers), and the dropout mask still comes from it"""
    def by_hand(x, key):
        k0, k1, m = key & 0xffffffff, key >> 32, 0xffffffff
        x = ((x ^ k0) * 0x9E3779B1) & m
        x ^= x >> 15
        x = ((x ^ k1) * 0x85EBCA6B) & m
        x ^= x >> 13
        x ^= x >> 16
        return x
    xs = [0, 1, 2, 0x7fffffff, 0x80000000, 0xffffffff, 12345]
    for key in (0, C.KEY_LO, C.KEY_HI, 0xffffffffffffffff):
        assert R.hash32(xs, key).tolist() == [by_hand(x, key) for x in xs]
    src = open(os.path.join(ROOT, "tests", "rowops_cases.py")).read() + open(os.path.join(ROOT, "tests", "batch_cases.py")).read()
    assert src.count("0x9E3779B1") == 1 and src.count("0x85EBCA6B") == 1                      # no second copy
    u, rnd = C.draw_values([0, 5], C.KEY_HI, 30522)
    assert float(u[1]) == (by_hand(10, C.KEY_HI) >> 8) / 2.0 ** 24 and int(rnd[1]) == (by_hand(11, C.KEY_HI) * 30522) >> 32


# ---- restatement against reference, planted defects --------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(REQUIRED))
def test_the_restated_kernels_equal_the_references_on_every_case(fam):
    for c in _cases(fam):
        ok, what = C.run_restated(c)
        assert ok, (what, c)


@pytest.mark.parametrize("fam,defect", sorted(CAUGHT_BY))
def test_a_planted_defect_is_rejected(fam, defect):
    names = CAUGHT_BY[(fam, defect)]
    must = [c for c in _cases(fam) if names is None or set(names) & set(_branch(c))]
    assert must, (fam, defect)
    rejected = []
    for c in _cases(fam):
        ok, what = C.run_restated(c, defect)
        if not ok:
            rejected.append(C.case_id(c))
        assert not (ok and c in must), (defect, "let through", c, _branch(c))
    print(f"\n{fam}/{defect}: rejected by {len(rejected)} of {len(_cases(fam))} cases ({len(must)} required): " + ", ".join(rejected))


def test_the_two_le_defects_exist_only_against_the_f32_constants():
    """module docstring: in double, `<=` and `<` are the same function of an f32 u at both thresholds"""
    e = C.edge_draws()
    near = np.concatenate([np.float32(v) + np.arange(-8, 9) * np.spacing(np.float32(v)) for v in (0.15, 0.12, 0.135)]).astype(np.float32)
    for u in np.concatenate([e, near]):
        p = float(u)
        assert p != 0.15 and p / 0.15 != 0.8 and p / 0.15 != 0.9
    assert int(C._mlm_action(np.float32([0.15]), "le_0.15")[0]) != 0 == int(C._mlm_action(np.float32([0.15]), None)[0])
    up = np.nextafter(np.float32(0.12), np.float32(1.0))
    assert int(C._mlm_action(np.array([up]), "le_0.8")[0]) == 1 and int(C._mlm_action(np.array([up]), None)[0]) == 2
    assert np.float32(0.15) in e and up in e


# ---- the draw stream's statistics, on the numpy hash --------------------------------------------------------------------------------
def test_the_draw_stream_is_well_distributed():
    B, S, V = 64, 473, 30522
    n = B * S
    u, rnd = C.draw_stream(C.KEY_HI, B, S, V)
    assert u.dtype == np.float32 and rnd.dtype == np.int32
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and int(rnd.min()) >= 0 and int(rnd.max()) < V
    assert np.array_equal(u.astype(np.float64) * 2 ** 24, np.round(u.astype(np.float64) * 2 ** 24))          # the 2^-24 grid
    share, mean_u, mean_r = float((u.astype(np.float64) < 0.15).mean()), float(u.astype(np.float64).mean()), float(rnd.astype(np.float64).mean()) / V
    print(f"\nshare u < 0.15: {share:.5f}   mean u: {mean_u:.5f}   mean rnd / vocab: {mean_r:.5f}   (n = {n})")
    assert abs(share - 0.15) < 4 * math.sqrt(0.15 * 0.85 / n)
    assert abs(mean_u - 0.5) < 4 * math.sqrt(1 / 12 / n) and abs(mean_r - 0.5) < 4 * math.sqrt(1 / 12 / n)
    u2, _ = C.draw_stream(C.KEY_HI + 1, B, S, V)
    assert not np.array_equal(u, u2) and abs(float(np.corrcoef(u.ravel(), u2.ravel())[0, 1])) < 4 / math.sqrt(n)
    a, b = C.draw_stream(C.KEY_HI, 2 * B, S, V), C.draw_stream(C.KEY_HI, S, B, V)
    assert np.array_equal(a[0][:B], u) and np.array_equal(b[1].ravel(), rnd.ravel())


# ---- host twins ------------------------------------------------------------------------------------------------------------------
def test_the_host_twins_agree_with_the_references_on_the_chain_cases():
    from medvill_amd import data
    for c in C.chain_cases():
        inp = C.chain_inputs(c)
        ref = C.chain_reference(c, inp)
        assert C.chain_twins(c, inp, ref) == [], c
        assert set(C.chain_buffers(c, ref)) | {"sel"} == set(ref), c
    # data.corrupt_tokens: the same selection rule and the same forced mask, on the draws its generator makes
    B, S, V = 96, 6, 30522
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(1000, V, (B, S), generator=gen)
    lengths = torch.tensor([(1, 2, 3, S)[b % 4] for b in range(B)])
    state = gen.get_state()
    out, labels = data.corrupt_tokens(ids, lengths, V, gen)
    gen.set_state(state)
    u = torch.rand((B, S), generator=gen)
    rnd = torch.randint(0, V, (B, S), generator=gen)
    ref = C._corrupt_plain(B, 0, S, ids.numpy(), lengths.numpy().astype(np.int32), u.numpy(), rnd.numpy().astype(np.int32), None, V)
    txt, lab = ref["input_txt"][0].reshape(B, S + 1), ref["txt_labels"][0].reshape(B, S + 3)
    forced = 0
    for b in range(B):
        n = int(lengths[b])
        assert out[b, :n].tolist() == txt[b, :n].tolist() and labels[b, :n].tolist() == lab[b, 2:2 + n].tolist(), b
        assert labels[b, n:].tolist() == [-100] * (S - n) and int(ref["counts"][0][b]) >= 1
        forced += int(not bool((u[b, :n] < 0.15).any()))
    assert forced >= 10                                        # the rule under test was exercised


# ---- argument rejects: every call returns before a launch ---------------------------------------------------------------------------
E_ARG, E_SHAPE = -1, -2
P = 0x1000          # a non-null address that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    import medvill_amd  # noqa: F401
    from medvill_amd import _lib
    return _lib.load()


def test_mlm_draws_rejects(lib):
    d = lambda key=7, B=2, S=8, V=100, u=P, r=P: lib.mv_mlm_draws(key, B, S, V, u, r, None)      # noqa: E731
    assert d(u=None) == E_ARG and d(r=None) == E_ARG
    for k in ("B", "S", "V"):
        assert d(**{k: 0}) == E_ARG and d(**{k: -3}) == E_ARG, k
    assert d(B=65536, S=32768) == E_SHAPE and d(B=2 ** 31 - 1, S=2) == E_SHAPE and d(B=46341, S=46341) == E_SHAPE     # B*S > 2^31-1


def test_mlm_corrupt_rejects(lib):
    names = ("ids", "lengths", "u", "rnd", "family", "input_txt", "segment", "txt_labels", "n_ids", "desc", "counts", "label_rows", "label_ids", "n_labels")

    def c(B=2, N=4, S=8, **k):
        a = {n: P for n in names}
        a.update(k)
        return lib.mv_mlm_corrupt(a["ids"], a["lengths"], a["u"], a["rnd"], a["family"], B, N, S, a["input_txt"], a["segment"], a["txt_labels"],
                                  a["n_ids"], a["desc"], a["counts"], a["label_rows"], a["label_ids"], a["n_labels"], None)
    for n in names:
        if n not in ("family", "desc", "label_rows", "label_ids", "n_labels"):                 # the nullable ones
            assert c(**{n: None}) == E_ARG, n
    assert c(B=0) == E_ARG and c(B=-1) == E_ARG and c(S=0) == E_ARG and c(S=-2) == E_ARG and c(N=-1) == E_ARG
    idx = ("label_rows", "label_ids", "n_labels")
    for keep in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):                                      # a partial index triple
        assert c(**{n: None for j, n in enumerate(idx) if j not in keep}) == E_ARG, keep
    assert c(B=65536, S=32768, N=0) == E_SHAPE and c(B=2 ** 20, S=1, N=2044) == E_SHAPE          # B*L > 2^31-1
    assert c(B=65536, S=32768, N=0, label_rows=None, label_ids=None, n_labels=None, family=None, desc=None) == E_SHAPE


def test_pack_plan_and_tail_perm_rejects(lib):
    p = lambda desc=P, B=2, L=64, cu=P, rowmap=P, inv=P: lib.mv_pack_plan(desc, B, L, cu, rowmap, inv, None)      # noqa: E731
    for k in ("desc", "cu", "rowmap", "inv"):
        assert p(**{k: None}) == E_ARG, k
    assert p(B=0) == E_ARG and p(B=-1) == E_ARG and p(L=0) == E_ARG and p(L=-64) == E_ARG
    assert p(B=65536, L=32768) == E_SHAPE and p(B=2, L=2 ** 30) == E_SHAPE
    t = lambda cu=P, B=2, L=64, sel=P, n_sel=4, perm=P, newpos=P, qlim=P, sel_new=P: \
        lib.mv_tail_perm(cu, B, L, sel, n_sel, perm, newpos, qlim, sel_new, None)                # noqa: E731
    for k in ("cu", "sel", "perm", "newpos", "qlim", "sel_new"):
        assert t(**{k: None}) == E_ARG, k
    assert t(B=0) == E_ARG and t(L=0) == E_ARG and t(n_sel=0) == E_ARG and t(n_sel=-1) == E_ARG and t(B=-2) == E_ARG
    assert t(L=C.TP_MAXL + 1) == E_SHAPE and t(L=2 ** 30) == E_SHAPE
