"""The classification bank without a GPU: the numpy restatements of tests/clf_bank_cases.py against data.ClassificationBank and
classification.metrics, the branches of mv_clf_assemble's launcher the case set reaches (its constants are read out of the sources), the
planted defects the sweep's comparison must catch, data.ClassificationBank's host side and the CPU-reachable half of the two entries' C
ABI (each validates its arguments before it touches the HIP runtime)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                                   # noqa: E402
from medvill_amd import _build, _lib                       # noqa: E402
from medvill_amd import classification as K_               # noqa: E402
import clf_bank_cases as C                                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mv_clf_assemble", "mv_clf_counts")
K = C.source_constants()
SMALL_COUNTS = [(n, c) for n, c in C.COUNT_CASES if n * c <= 70000]        # the rest run on the GPU only (the rule is the same)


def _exact(a, b):
    """The sweep's comparison: same dtype, same shape, same bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _cases():
    out = []
    for case in C.SWEEP:
        bank = C.sweep_bank(case)
        out.append((case, bank, C.batch_idx(bank, case[0], seed=case[0] + case[2])))
    return out


# ------------------------------------------------------------------------------------------------ the launcher's branches and caps
def test_constants_are_read_from_the_source():
    assert {"NT", "MAX_T", "MAX_C", "MAX_ELEMS", "RPT", "TILE", "NCOUNT", "VEC_BYTES", "UNROLL", "CHUNK_BYTES", "MAX_CHUNKS"} <= set(K)
    assert K["MAX_C"] == 1024 == mv.data.CLF_MAX_CLASSES and K["MAX_ELEMS"] == 1 << 21 and K["NCOUNT"] == C.NCOUNT == 7
    assert K["TILE"] == K["NT"] * K["RPT"] and K["TILE"] % 4 == 0
    from medvill_amd import hip_ops as ops
    assert (ops.CLF_MAX_CLASSES, ops.CLF_MAX_ELEMS, ops.CLF_NCOUNT) == (K["MAX_C"], K["MAX_ELEMS"], K["NCOUNT"])


def test_every_launcher_branch_but_large_chunks_is_reached_by_a_sweep_case():
    seen = set()
    for case in C.SWEEP:
        B, Cn, T, N, F, dtn, fam, guard = case
        item = C.ITEMSIZE[dtn]
        plan = C.launch_plan(N, F, item, aligned=(guard * item) % K["VEC_BYTES"] == 0, k=K)
        assert plan["chunks"] <= K["MAX_CHUNKS"] and plan["chunk"] * plan["chunks"] >= N * F > plan["chunk"] * (plan["chunks"] - 1)
        seen |= plan["branches"]
    assert seen == C.ALL_BRANCHES - {"large_chunks"}, C.ALL_BRANCHES ^ seen
    assert {c[1] for c in C.SWEEP} == set(C.CLASS_COUNTS) | {14} and set(C.CLASS_COUNTS) == {1, 31, 32, 33, K["MAX_C"]}
    assert {c[2] for c in C.SWEEP} == {2, 46, K["MAX_T"]} and {c[5] for c in C.SWEEP} == {"f32", "bf16", "f16"}
    assert {c[6] for c in C.SWEEP} == {None, "per"}
    # the counts: every n x C the request names, tile edges on both sides of a pair, one case past a block's tile in both lists
    assert set(C.COUNT_CASES) == {(n, c) for n in (1, 2, 63, 64, 65, 257, 1000) for c in (1, 31, 32, 33, 1024)}
    sizes = {n * c for n, c in C.COUNT_CASES}
    assert {K["TILE"] - 32, K["TILE"], K["TILE"] + 32} <= sizes and max(sizes) <= K["MAX_ELEMS"]
    case = C.make_counts_case(257, 1024)
    y = case["hot"][np.clip(case["idx"], 0, len(case["hot"]) - 1)]
    assert y.sum() > K["TILE"] and (~y).sum() > K["TILE"]


def test_the_case_sets_hold_the_named_situations():
    kinds = set()
    for case, bank, idx in _cases():
        B, Cn, T = case[:3]
        n = len(bank["txt_len"])
        assert bank["txt_len"][0] == 1 and bank["txt_len"][1] == T                                 # length 1 and length T
        assert not bank["hot"][0].any() and bank["hot"][1].all()                                   # no label; every class
        assert (bank["s_img"][2:5] == 0).sum() >= 1 and bank["s_img"][3] >= 3 and bank["s_img"][4] < 0   # shared, past, below
        kinds |= {"repeated"} if len(set(idx.tolist())) < B else set()
        kinds |= {"below"} if (idx < 0).any() else set()
        kinds |= {"past"} if (idx >= n).any() else set()
    for n, Cn in SMALL_COUNTS:
        case = C.make_counts_case(n, Cn)
        cnt = C.counts(case["probs"], case["idx"], case["lab_bits"], Cn)
        n_items = len(case["hot"])
        kinds |= {"repeated"} if len(set(np.clip(case["idx"], 0, n_items - 1).tolist())) < n else set()
        kinds |= {"below"} if (case["idx"] < 0).any() else set()
        kinds |= {"past"} if (case["idx"] >= n_items).any() else set()
        if Cn >= 3 and n >= 2:
            assert cnt[0, C.N_POS] == 0 and cnt[Cn - 1, C.N_NEG] == 0
            kinds |= {"no_positive", "no_negative"}
        for v in C.EXACT_PROBS:
            kinds |= {f"exact_{v}"} if (case["probs"] == v).any() else set()
        kinds |= {"ties_across_labels"} if cnt[Cn, C.EQ] > 0 else set()
        assert (cnt[:, C.N_POS] + cnt[:, C.N_NEG] == [n] * Cn + [n * Cn]).all()
    assert kinds == {"repeated", "below", "past", "no_positive", "no_negative", "exact_0.0", "exact_0.5", "exact_1.0",
                     "ties_across_labels"}, kinds


# ------------------------------------------------------------------------------------------------ the restatement against the package
def _host_bank(bank, Cn, ragged):
    cb = mv.data.ClassificationBank(device="cpu", n_classes=Cn)
    cb.add_samples(torch.from_numpy(bank["txt_ids"]), torch.from_numpy(bank["txt_len"]), bank["classes"] if ragged else bank["hot"],
                   np.clip(bank["s_img"], 0, None))
    return cb


def test_restated_targets_and_bits_equal_the_bank():
    for k, (case, bank, idx) in enumerate(_cases()):
        Cn = case[1]
        cb = _host_bank(bank, Cn, ragged=k % 2 == 0)
        assert cb.lab_bits.dtype == torch.int32 and _exact(cb.lab_bits.numpy(), bank["lab_bits"])
        inside = np.clip(idx, 0, len(bank["txt_len"]) - 1)
        got = C.assemble(bank, idx, Cn)["target"]
        assert _exact(got, cb.dense_targets(inside).numpy())
        for i, d in enumerate(inside):
            assert _exact(got[i], C.reference_target(bank["classes"][d], Cn))


@pytest.mark.parametrize("n,Cn", SMALL_COUNTS)
def test_restated_metrics_equal_the_package_bit_for_bit(n, Cn):
    case = C.make_counts_case(n, Cn)
    cnt = C.counts(case["probs"], case["idx"], case["lab_bits"], Cn)
    y = case["hot"][np.clip(case["idx"], 0, len(case["hot"]) - 1)].astype(np.float32)
    want = K_.metrics(torch.from_numpy(case["probs"]), torch.from_numpy(y))
    # (macro F1: the restated per-class values through torch's reduction -- see clf_bank_cases.metrics)
    torch_mean = lambda v: float(torch.from_numpy(np.ascontiguousarray(v)).mean())
    # numpy's own order of additions: either sum of C values in [0, 1] is within (C - 1) u of the exact one (u = eps / 2), relative,
    # and the mean is at most 1 -- so the two differ by less than 2 C u = C eps
    assert abs(C.metrics(cnt)["macro_f1"] - want["macro_f1"]) <= Cn * np.finfo(np.float64).eps
    for got in (C.metrics(cnt, mean=torch_mean), K_.metrics_from_counters(torch.from_numpy(cnt))):
        assert set(got) == set(want)
        for k in want:
            assert got[k] == want[k], (k, got[k], want[k])
    # the counters accumulate, and twice the counts give the same ratios
    twice = C.counts(case["probs"], case["idx"], case["lab_bits"], Cn, counters=cnt)
    assert (twice == 2 * cnt).all()


def test_metrics_from_counters_handles_missing_label_values():
    cnt = np.zeros((3, 7), np.int64)
    cnt[0] = (2, 3, 4, 1, 1, 1, 1)                      # AUROC (8 + 1) / 12, F1 2 / 4
    cnt[1] = (0, 5, 0, 0, 0, 0, 0)                      # no positive: AUROC 0, F1 0 on a zero denominator
    cnt[2] = (2, 8, 10, 2, 1, 1, 1)
    m = K_.metrics_from_counters(cnt)
    assert m["auroc_per_class"] == [0.75, 0.0] and m["macro_auroc"] == 0.375 and m["micro_auroc"] == 22 / 32
    assert m["macro_f1"] == 0.25 and m["micro_f1"] == 0.5
    assert K_.metrics_from_counters(np.zeros((2, 7), np.int64))["micro_f1"] == 0.0
    with pytest.raises(ValueError):
        K_.metrics_from_counters(np.zeros((3, 6), np.int64))


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("defect,keys", [("bit_from_wrong_word", ("target",)), ("len_off_by_one", ("segment", "desc")),
                                         ("image_from_idx", ("feats", "pos"))])
def test_the_sweeps_comparison_catches_a_planted_assemble_defect(defect, keys):
    caught = 0
    for case, bank, idx in _cases():
        good, bad = C.assemble(bank, idx, case[1]), C.assemble(bank, idx, case[1], defect=defect)
        assert all(_exact(good[k], bad[k]) for k in good if k not in keys)
        hit = any(not _exact(good[k], bad[k]) for k in keys)
        if defect == "bit_from_wrong_word":
            assert hit == (case[1] > 32), case                                 # every case with a second word
        caught += int(hit)
    assert caught >= 3, defect


@pytest.mark.parametrize("defect,cols", [("ties_as_wins", (C.GT, C.EQ)), ("threshold_ge", (C.TP, C.FP, C.FN)),
                                         ("micro_from_class_sums", (C.GT, C.EQ))])
def test_the_sweeps_comparison_catches_a_planted_counts_defect(defect, cols):
    caught = 0
    for n, Cn in SMALL_COUNTS:
        case = C.make_counts_case(n, Cn)
        good = C.counts(case["probs"], case["idx"], case["lab_bits"], Cn)
        bad = C.counts(case["probs"], case["idx"], case["lab_bits"], Cn, defect=defect)
        others = [k for k in range(C.NCOUNT) if k not in cols]
        assert _exact(good[:, others], bad[:, others])
        if defect == "micro_from_class_sums":
            assert _exact(good[:Cn], bad[:Cn])
        caught += int(not _exact(good, bad))
    assert caught >= 10, defect


# ------------------------------------------------------------------------------------------------ ABI
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "medvill.h")).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(mv_clf_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_new_symbols_are_declared_exported_and_prototyped():
    decl = _declared()
    assert set(decl) == set(NEW)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and len(_lib.PROTOTYPES[name]) == decl[name], name
    assert "mv_clf_bank.hip" in _build.SOURCES
    assert re.search(r"#define\s+MV_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "medvill.h")).read()) and _lib.ABI_VERSION == 6
    from medvill_amd import hip_ops as ops
    assert callable(ops.clf_assemble) and callable(ops.clf_counts)
    assert callable(mv.CXRBertForClassification.fit_step) and callable(mv.CXRBertForClassification.evaluate)
    assert '#include "mv_bank.h"' in open(C.HIP_SOURCE).read() and "copy_chunk(" in open(C.HIP_SOURCE).read()     # the shared gather


E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
PTR = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below must return before a launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_clf_assemble_rejects(lib):
    def asm(**k):
        g = lambda name, default=PTR: k.get(name, default)
        return lib.mv_clf_assemble(g("ids"), g("len"), g("s_img"), g("bits"), g("n", 5), g("img"), g("dt", 2), g("ipos"), g("n_img", 3),
                                   g("idx"), g("family", None), g("B", 3), g("N", 3), g("T", 6), g("F", 8), g("C", 14), g("txt"), g("seg"),
                                   g("desc"), g("feats"), g("pos"), g("target"), None)
    for name in ("ids", "len", "s_img", "bits", "img", "ipos", "idx", "txt", "seg", "desc", "feats", "pos", "target"):
        assert asm(**{name: None}) == E_ARG, name
    for name in ("n", "n_img", "B", "N", "T", "F", "C"):
        assert asm(**{name: 0}) == E_ARG and asm(**{name: -2}) == E_ARG, name
    assert asm(dt=3) == E_DTYPE and asm(dt=-1) == E_DTYPE
    assert asm(T=K["MAX_T"] + 1) == E_SHAPE and asm(C=K["MAX_C"] + 1) == E_SHAPE
    assert asm(N=1 << 16, F=1 << 15) == E_SHAPE and asm(B=1 << 21, T=1024) == E_SHAPE          # N F, B T = 2^31


def test_clf_counts_rejects(lib):
    def cnt(**k):
        g = lambda name, default=PTR: k.get(name, default)
        return lib.mv_clf_counts(g("probs"), g("ld", 16), g("idx"), g("n", 10), g("bits"), g("n_items", 5), g("C", 14), g("counters"), None)
    for name in ("probs", "idx", "bits", "counters"):
        assert cnt(**{name: None}) == E_ARG, name
    for name in ("n", "n_items", "C"):
        assert cnt(**{name: 0}) == E_ARG and cnt(**{name: -1}) == E_ARG, name
    assert cnt(ld=13) == E_ARG and cnt(ld=0) == E_ARG                                          # a row shorter than its classes
    assert cnt(C=K["MAX_C"] + 1, ld=2048) == E_SHAPE
    assert cnt(n=K["MAX_ELEMS"] + 1, C=1) == E_SHAPE                                           # n C = 2^21 + 1
    assert cnt(n=(K["MAX_ELEMS"] >> 10) + 1, C=1024, ld=1024) == E_SHAPE and cnt(n=1 << 30, C=1024, ld=1024) == E_SHAPE


# ------------------------------------------------------------------------------------------------ ClassificationBank, host side
def test_bits_from_multi_hot_and_ragged_labels_and_the_host_copies():
    cb = mv.data.ClassificationBank(device="cpu", n_classes=33)
    ids = torch.zeros((4, 5), dtype=torch.int64)
    cb.add_samples(ids, [1, 5, 3, 2], [[3, 32, 3], None, [], np.array([31, 0])])
    hot = np.zeros((2, 33), np.float32)
    hot[0, [1, 32]], hot[1, 31] = (1.0, 0.6), 0.5                            # above 0.5 is set; 0.5 is not
    cb.add_samples(ids[:2], [2, 2], hot, image_item=[1, 0])                  # a second part, as a multi-hot array
    assert cb.n_samples == cb.n_texts == 6 and cb.n_words == 2
    assert cb.lab_bits.dtype == torch.int32 and cb.lab_bits.tolist() == [[8, 1], [0, 0], [0, 0], [-2 ** 31 + 1, 0], [2, 1], [0, 0]]
    assert _exact(cb.lab_bits.numpy(), cb._bits_host.numpy())
    assert cb.s_img.dtype == torch.int32 and cb.s_img.tolist() == [0, 1, 2, 3, 1, 0] == cb._s_img_host.tolist()     # None: item i is image i
    assert cb._len_host.tolist() == [1, 5, 3, 2, 2, 2]
    t = cb.dense_targets([0, 3, 4, 0])
    assert t.dtype == torch.float32 and tuple(t.shape) == (4, 33) and torch.equal(t[0], t[3])
    assert t[0].nonzero().view(-1).tolist() == [3, 32] and t[1].nonzero().view(-1).tolist() == [0, 31] and t[2].nonzero().view(-1).tolist() == [1, 32]
    cb.add_images((torch.zeros(4, 3, 8), torch.zeros(4, 3, dtype=torch.int64)))
    d = cb.host_descriptors(cb.host_idx([1, 0, 3]), torch.tensor([4, 1, 2], dtype=torch.int32))
    assert d.dtype == torch.int32 and d.tolist() == [[4, 5, 10], [1, 5, 6], [2, 5, 7]]


def test_pos_weight_is_the_reference_expression():
    g = np.random.default_rng(5)
    hot = g.random((37, 14)) < 0.3
    hot[0], hot[1] = True, False
    hot[:, 5] = True                                                         # no negative: freq / 0 = inf, ** -1 = 0
    cb = mv.data.ClassificationBank(device="cpu", n_classes=14)
    cb.add_samples(torch.zeros((37, 3), dtype=torch.int64), [1] * 37, hot)
    freqs = [int(hot[:, c].sum()) for c in range(14)]
    negative = [37 - f for f in freqs]
    want = (torch.FloatTensor(freqs) / torch.FloatTensor(negative)) ** -1    # main.py:96-98
    got = cb.pos_weight()
    assert got.dtype == torch.float32 and torch.equal(got, want) and got[5] == 0.0
    assert _exact(got.numpy(), C.reference_pos_weight(hot))
    hot[:, 2] = False
    cb2 = mv.data.ClassificationBank(device="cpu", n_classes=14)
    with pytest.raises(ValueError, match="empty"):
        cb2.pos_weight()
    cb2.add_samples(torch.zeros((37, 3), dtype=torch.int64), [1] * 37, hot)
    with pytest.raises(ValueError, match="no positive"):
        cb2.pos_weight()


def test_classification_bank_refusals_on_the_host():
    cb = mv.data.ClassificationBank(device="cpu", n_classes=10)
    ids = torch.zeros((2, 5), dtype=torch.int64)
    ok = dict(ids=ids, lengths=[1, 5], labels=[[1], [2, 2]], image_item=[0, 1])
    bad = [dict(labels=[[10], [2]]), dict(labels=[[-1], [2]]), dict(labels=[[1.5], [2]]), dict(labels=[[1]]), dict(labels=None),
           dict(labels=np.zeros((2, 9))), dict(labels=torch.zeros((3, 10))), dict(image_item=[0, -1]), dict(image_item=[0.0, 1.0]),
           dict(image_item=[0]), dict(lengths=[1, 6]), dict(lengths=[1]), dict(ids=torch.zeros(5, dtype=torch.int64))]
    for over in bad:
        with pytest.raises(ValueError):
            cb.add_samples(**{**ok, **over})
        assert cb.n_samples == 0 and cb.n_texts == 0 and cb._bits_host.shape[0] == 0, over      # a refused call adds nothing
    for c in (0, -1, 1025):
        with pytest.raises(ValueError):
            mv.data.ClassificationBank(device="cpu", n_classes=c)
    assert mv.data.ClassificationBank(device="cpu", n_classes=1024).n_words == 32
    with pytest.raises(ValueError, match="empty"):
        cb.assemble([0])
    cb.add_samples(**ok)
    with pytest.raises(ValueError, match="empty"):
        cb.assemble([0])
    cb.add_images((torch.zeros(1, 3, 8), torch.zeros(1, 3, dtype=torch.int64)))
    with pytest.raises(IndexError):
        cb.assemble([0, 2])
    with pytest.raises(IndexError):
        cb.assemble([-1])
    with pytest.raises(IndexError):
        cb.dense_targets([2])
    with pytest.raises(ValueError, match="image"):                          # sample 1 names image 1: not in the bank yet
        cb.assemble([0, 1])
    cb.add_images((torch.zeros(1, 3, 8), torch.zeros(1, 3, dtype=torch.int64)))
    with pytest.raises(ValueError, match="mode"):
        cb.assemble([0, 1], mode="full")
    with pytest.raises(ValueError, match="mode"):
        cb.assemble([0, 1], mode=["bi"])
    with pytest.raises(ValueError):
        cb.assemble([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # a missing kernel is an error, not a host loop
        cb.assemble([0, 1])
    cb.add_texts(ids, [1, 1])
    with pytest.raises(ValueError, match="add_samples"):
        cb.assemble([0])
