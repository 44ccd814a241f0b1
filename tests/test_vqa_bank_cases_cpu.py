"""The VQA bank without a GPU: the numpy restatements of tests/vqa_bank_cases.py against data.VqaBank.dense_targets and a direct scatter_
per question, the branches of mv_vqa_assemble's launcher the case set reaches (its constants are read out of csrc/mv_bank.h), the
planted defects the sweep's comparison must catch, data.VqaBank's host side and the CPU-reachable half of the two entries' C ABI (each
validates its arguments before it touches the HIP runtime)."""
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
from medvill_amd.vqa import vqa_metrics                    # noqa: E402
import vqa_bank_cases as C                                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mv_vqa_assemble", "mv_vqa_score")
K = C.source_constants()


def _exact(a, b):
    """The sweep's comparison: same dtype, same shape, same bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _small_cases():
    """(case, bank, idx, pred) of every sweep case but the one whose rows are tens of megabytes (its rule is the same)."""
    out = []
    for case in C.SWEEP:
        B, A, T, N, F = case[:5]
        if N * F > 1 << 20:
            continue
        bank = C.sweep_bank(case)
        idx = C.batch_idx(bank, B, seed=B + T)
        out.append((case, bank, idx, C.batch_pred(bank, idx, A, seed=A)))
    return out


# ------------------------------------------------------------------------------------------------ the launcher's branches and caps
def test_constants_are_read_from_the_source():
    assert {"NT", "MAX_T", "MAX_G", "VEC_BYTES", "UNROLL", "CHUNK_BYTES", "MAX_CHUNKS"} <= set(K)
    assert K["CHUNK_BYTES"] % (K["VEC_BYTES"] * K["UNROLL"] * K["NT"]) == 0        # a full chunk is whole unrolled rounds


def test_every_launcher_branch_is_reached_by_a_sweep_case():
    seen = set()
    for case in C.SWEEP:
        B, A, T, N, F, dtn, fam, grp, guard = case
        item = C.ITEMSIZE[dtn]
        plan = C.launch_plan(N, F, item, aligned=(guard * item) % K["VEC_BYTES"] == 0, k=K)
        assert plan["chunks"] <= K["MAX_CHUNKS"] and plan["chunk"] * plan["chunks"] >= N * F > plan["chunk"] * (plan["chunks"] - 1)
        if plan["vec"]:
            assert plan["chunk"] % (K["VEC_BYTES"] // item) == 0
        seen |= plan["branches"]
    assert seen == C.ALL_BRANCHES, C.ALL_BRANCHES - seen
    # the values the request names all occur, and T reaches the kernel's cap
    assert {c[0] for c in C.SWEEP} >= {1, 3, 64} and {c[1] for c in C.SWEEP} == {1, 17, 458}
    assert {c[2] for c in C.SWEEP} == {2, 46, K["MAX_T"]} and {c[5] for c in C.SWEEP} == {"f32", "bf16", "f16"}
    assert {c[6] for c in C.SWEEP} == {None, "per"} and {c[7] for c in C.SWEEP} == {None, K["MAX_G"]}
    # a row of both element sizes on each side of the one-chunk / many-chunks line
    for item in (2, 4):
        sides = {C.launch_plan(c[3], c[4], item, True, K)["chunks"] > 1 for c in C.SWEEP if C.ITEMSIZE[c[5]] == item}
        assert sides == {False, True}, item


def test_the_case_set_holds_the_named_situations():
    kinds = set()
    for case, bank, idx, pred in _small_cases():
        B, A = case[:2]
        n = len(bank["txt_len"])
        assert bank["txt_len"][0] == 1 and bank["txt_len"][1] == case[2]                           # length 1 and length T
        assert bank["ans_ptr"][1] == 0 and bank["ans_ptr"][2] - bank["ans_ptr"][1] == 1            # no answers; one answer
        two = bank["ans_label"][bank["ans_ptr"][2]:bank["ans_ptr"][3]].tolist()
        assert two[0] == two[-1] and len(two) >= 2                                                 # a duplicated label
        assert (bank["q_img"][2:5] == 0).sum() >= 1 and bank["q_img"][3] >= 3 and bank["q_img"][4] < 0   # shared, past, below
        assert set(bank["ans_type"].tolist()) == {0, 1, 2} and 5 not in bank["group"].tolist()
        if len(set(idx.tolist())) < B:
            kinds.add("repeated")
        if (idx < 0).any():
            kinds.add("below")
        if (idx >= n).any():
            kinds.add("past")
        sc, _ = C.score(bank, pred, idx, 8)
        for i, q in enumerate(idx):
            d = C.clamp(q, 0, n - 1)
            mine = bank["ans_label"][bank["ans_ptr"][d]:bank["ans_ptr"][d + 1]].tolist()
            kinds.add("listed" if pred[i] in mine else "unlisted")
            if pred[i] == A - 1 and pred[i] in mine:
                kinds.add("last_column_hit")
            if d == 2 and pred[i] == mine[0]:
                kinds.add("duplicate_hit")
                assert sc[i] == np.float32(0.9)                                                    # the later score
    assert kinds == {"repeated", "below", "past", "listed", "unlisted", "last_column_hit", "duplicate_hit"}, kinds


# ------------------------------------------------------------------------------------------------ the restatement against the reference
def _host_bank(bank, A, upto=None):
    vb = mv.data.VqaBank(device="cpu", n_answers=A)
    n = len(bank["txt_len"]) if upto is None else upto
    q_img = np.clip(bank["q_img"][:n], 0, None)
    vb.add_questions(torch.from_numpy(bank["txt_ids"][:n]), torch.from_numpy(bank["txt_len"][:n]), q_img, bank["labels"][:n],
                     bank["scores"][:n], bank["ans_type"][:n].tolist(), group=bank["group"][:n].tolist())
    return vb


def test_restated_targets_equal_dense_targets_and_a_direct_scatter():
    for case, bank, idx, pred in _small_cases():
        A = case[1]
        n = len(bank["txt_len"])
        vb = _host_bank(bank, A)
        inside = np.clip(idx, 0, n - 1)
        got = C.assemble(bank, idx, A)["target"]
        assert _exact(got, vb.dense_targets(inside).numpy())
        for i, d in enumerate(inside):
            direct = torch.zeros(A)
            if bank["labels"][d]:
                direct.scatter_(0, torch.tensor(bank["labels"][d], dtype=torch.int64), torch.tensor(bank["scores"][d], dtype=torch.float32))
            assert _exact(got[i], direct.numpy()) and _exact(got[i], C.reference_target(bank["labels"][d], bank["scores"][d], A))
        # the score of a prediction is the dense target's value at its column (model.py:1007-1012, 1023)
        sc, _ = C.score(bank, pred, idx, 8)
        assert _exact(sc, got[np.arange(len(idx)), pred])
        assert vb.ans_ptr.tolist() == bank["ans_ptr"].tolist() and vb.ans_label.tolist() == bank["ans_label"].tolist()


def test_restated_metrics_equal_the_package_and_give_nan_for_an_empty_split():
    case, bank, idx, pred = _small_cases()[2]
    _, cnt = C.score(bank, pred, idx, 8)
    _, cnt = C.score(bank, pred, idx, 8, counters=cnt)                                           # accumulated: twice the sums
    _, once = C.score(bank, pred, idx, 8)
    assert (cnt == 2 * once).all() and cnt[5].sum() == 0 and cnt[:, :, 1].sum() == 2 * len(idx)
    a, b = vqa_metrics(torch.from_numpy(cnt)), C.metrics(cnt)
    assert set(a) == set(b) == {"acc", "closed_acc", "open_acc", "n", "closed_n", "open_n", "by_group"}
    assert set(a["by_group"]) == set(b["by_group"]) and 5 not in a["by_group"]
    for x, y in [(a, b)] + [(a["by_group"][g], b["by_group"][g]) for g in a["by_group"]]:
        for k in ("acc", "closed_acc", "open_acc", "n", "closed_n", "open_n"):
            assert x[k] == y[k] or (np.isnan(x[k]) and np.isnan(y[k])), k
    only_open = np.zeros((8, 3, 2), np.int64)
    only_open[0, 1] = (C.fx(0.6), 1)
    m = vqa_metrics(torch.from_numpy(only_open))
    assert np.isnan(m["closed_acc"]) and m["open_acc"] == m["acc"] == float(np.float32(0.6)) and m["closed_n"] == 0


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("defect,keys", [("first_duplicate", ("target",)), ("len_off_by_one", ("segment", "desc")),
                                         ("segment_ones", ("segment",)), ("image_from_idx", ("feats", "pos"))])
def test_the_sweeps_comparison_catches_a_planted_assemble_defect(defect, keys):
    caught = 0
    for case, bank, idx, pred in _small_cases():
        good, bad = C.assemble(bank, idx, case[1]), C.assemble(bank, idx, case[1], defect=defect)
        assert all(_exact(good[k], bad[k]) for k in good if k not in keys)
        caught += int(any(not _exact(good[k], bad[k]) for k in keys))
    assert caught >= 3, defect


@pytest.mark.parametrize("defect", ["slot_swapped", "fx_truncated"])
def test_the_sweeps_comparison_catches_a_planted_score_defect(defect):
    caught = 0
    for case, bank, idx, pred in _small_cases():
        (s0, c0), (s1, c1) = C.score(bank, pred, idx, 8), C.score(bank, pred, idx, 8, defect=defect)
        assert _exact(s0, s1)
        caught += int(not _exact(c0, c1))
    assert caught >= 3, defect
    assert C.fx(1e-6) != C.fx(1e-6, "fx_truncated") and C.fx(0.6) == C.fx(0.6, "fx_truncated") == 2576980480


# ------------------------------------------------------------------------------------------------ ABI
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "medvill.h")).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(mv_vqa_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_new_symbols_are_declared_exported_and_prototyped():
    decl = _declared()
    assert set(decl) == set(NEW)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and len(_lib.PROTOTYPES[name]) == decl[name], name
    assert "mv_vqa_bank.hip" in _build.SOURCES
    assert re.search(r"#define\s+MV_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "medvill.h")).read()) and _lib.ABI_VERSION == 6
    from medvill_amd import hip_ops as ops
    assert callable(ops.vqa_assemble) and callable(ops.vqa_score) and ops.VQA_MAX_GROUPS == K["MAX_G"] == mv.data.VQA_GROUPS
    assert callable(mv.CXRBertForVQA.fit_step) and callable(mv.CXRBertForVQA.evaluate)


E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
PTR = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below must return before a launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_vqa_assemble_rejects(lib):
    def asm(**k):
        g = lambda name, default=PTR: k.get(name, default)
        return lib.mv_vqa_assemble(g("ids"), g("len"), g("q_img"), g("n", 5), g("ptr"), g("lab"), g("sc"), g("nnz", 7), g("type"), g("img"),
                                   g("dt", 2), g("ipos"), g("n_img", 3), g("idx"), g("family", None), g("B", 3), g("N", 3), g("T", 6),
                                   g("F", 8), g("A", 17), g("txt"), g("seg"), g("desc"), g("feats"), g("pos"), g("target"), g("otype"), None)
    for name in ("ids", "len", "q_img", "ptr", "lab", "sc", "type", "img", "ipos", "idx", "txt", "seg", "desc", "feats", "pos", "target",
                 "otype"):
        assert asm(**{name: None}) == E_ARG, name
    for name in ("n", "n_img", "B", "N", "T", "F", "A"):
        assert asm(**{name: 0}) == E_ARG and asm(**{name: -2}) == E_ARG, name
    assert asm(nnz=-1) == E_ARG
    assert asm(dt=3) == E_DTYPE and asm(dt=-1) == E_DTYPE
    assert asm(T=K["MAX_T"] + 1) == E_SHAPE
    assert asm(N=1 << 16, F=1 << 15) == E_SHAPE and asm(B=1 << 21, T=1024) == E_SHAPE          # N F, B T = 2^31


def test_vqa_score_rejects(lib):
    def sc(**k):
        g = lambda name, default=PTR: k.get(name, default)
        return lib.mv_vqa_score(g("pred"), g("idx"), g("B", 4), g("n", 5), g("ptr"), g("lab"), g("sc"), g("nnz", 7), g("type"),
                                g("group", None), g("G", 8), g("score", None), g("counters"), None)
    for name in ("pred", "idx", "ptr", "lab", "sc", "type", "counters"):
        assert sc(**{name: None}) == E_ARG, name
    for name in ("B", "n", "G"):
        assert sc(**{name: 0}) == E_ARG and sc(**{name: -1}) == E_ARG, name
    assert sc(nnz=-1) == E_ARG
    assert sc(G=K["MAX_G"] + 1) == E_SHAPE and sc(G=K["MAX_G"] + 1, group=PTR) == E_SHAPE


# ------------------------------------------------------------------------------------------------ VqaBank, host side
def test_type_mapping_with_the_trailing_space_variants():
    given = ["CLOSED", "CLOSED ", "OPEN", "OPEN ", " OPEN", "closed", "", 0, 1, 2, -1, None, torch.tensor(1), np.int64(0), 1.5]
    want = [0, 0, 1, 1, 2, 2, 2, 0, 1, 2, 2, 2, 1, 0, 2]
    assert [mv.data.vqa_answer_type(t) for t in given] == want
    assert [C.answer_type(t) for t in given[:12]] == want[:12]
    vb = mv.data.VqaBank(device="cpu", n_answers=4)
    vb.add_questions(torch.zeros((len(given), 3), dtype=torch.int64), [1] * len(given), [0] * len(given), [None] * len(given),
                     [None] * len(given), given)
    assert vb.ans_type.dtype == torch.int32 and vb.ans_type.tolist() == want


def test_csr_from_ragged_and_none_answers_and_the_host_copies():
    vb = mv.data.VqaBank(device="cpu", n_answers=10)
    ids = torch.zeros((4, 5), dtype=torch.int64)
    vb.add_questions(ids, [1, 5, 3, 2], [2, 0, 0, 1], [[3, 9, 3], None, [], np.array([0])], [[0.3, 1.0, 0.9], None, [], torch.tensor([0.6])],
                     ["CLOSED", "OPEN ", "x", 1], group=[0, 7, 3, 3])
    vb.add_questions(ids[:2], [2, 2], [5, 1], [torch.tensor([4, 5]), None], [np.array([1.0, 0.5], np.float32), None], [0, 0])     # a second part
    assert vb.n_questions == vb.n_texts == 6 and vb.n_answers == 10
    assert vb.ans_ptr.dtype == torch.int32 and vb.ans_ptr.tolist() == [0, 3, 3, 3, 4, 6, 6]
    assert vb.ans_label.dtype == torch.int32 and vb.ans_label.tolist() == [3, 9, 3, 0, 4, 5]
    assert vb.ans_score.dtype == torch.float32 and vb.ans_score.tolist() == [np.float32(v) for v in (0.3, 1.0, 0.9, 0.6, 1.0, 0.5)]
    assert vb.q_img.dtype == torch.int32 and vb.q_img.tolist() == [2, 0, 0, 1, 5, 1] == vb._q_img_host.tolist()
    assert vb.ans_type.tolist() == [0, 1, 2, 1, 0, 0] and vb.group.dtype == torch.int32 and vb.group.tolist() == [0, 7, 3, 3, 0, 0]
    assert vb._len_host.tolist() == [1, 5, 3, 2, 2, 2]
    t = vb.dense_targets([0, 1, 4, 0])
    assert t.dtype == torch.float32 and tuple(t.shape) == (4, 10)
    assert t[0].tolist() == [0, 0, 0, np.float32(0.9), 0, 0, 0, 0, 0, 1.0] and torch.equal(t[0], t[3])      # the later 0.9 wins
    assert float(t[1].abs().sum()) == 0.0 and t[2, 4] == 1.0 and t[2, 5] == 0.5
    # the host descriptors: {family, N+2, N+2+len} from the host lengths
    vb.add_images((torch.zeros(6, 3, 8), torch.zeros(6, 3, dtype=torch.int64)))
    h = vb.host_idx([1, 0, 3])
    d = vb.host_descriptors(h, torch.tensor([4, 1, 2], dtype=torch.int32))
    assert d.dtype == torch.int32 and d.tolist() == [[4, 5, 10], [1, 5, 6], [2, 5, 7]]


def test_vqa_bank_refusals_on_the_host():
    vb = mv.data.VqaBank(device="cpu", n_answers=10)
    ids = torch.zeros((2, 5), dtype=torch.int64)
    ok = dict(ids=ids, lengths=[1, 5], image_item=[0, 1], labels=[[1], [2, 2]], scores=[[1.0], [0.5, 0.6]], ans_type=[0, 1])
    bad = [dict(labels=[[10], [2, 2]]), dict(labels=[[-1], [2, 2]]), dict(scores=[[1.0], [0.5]]), dict(scores=[[1.0], None]),
           dict(scores=[[float("nan")], [0.5, 0.6]]), dict(scores=[[1.0], [float("inf"), 0.6]]), dict(group=[0, 8]), dict(group=[-1, 0]),
           dict(image_item=[0, -1]), dict(lengths=[1, 6]), dict(ans_type=[0])]
    for over in bad:
        with pytest.raises(ValueError):
            vb.add_questions(**{**ok, **over})
        assert vb.n_questions == 0 and vb.n_texts == 0 and vb.ans_ptr.tolist() == [0], over      # a refused call adds nothing
    with pytest.raises(ValueError):
        mv.data.VqaBank(device="cpu", n_answers=0)
    with pytest.raises(ValueError, match="empty"):
        vb.assemble([0])
    vb.add_questions(**ok)
    with pytest.raises(ValueError, match="empty"):
        vb.assemble([0])
    vb.add_images((torch.zeros(1, 3, 8), torch.zeros(1, 3, dtype=torch.int64)))
    with pytest.raises(IndexError):
        vb.assemble([0, 2])
    with pytest.raises(IndexError):
        vb.assemble([-1])
    with pytest.raises(IndexError):
        vb.dense_targets([2])
    with pytest.raises(ValueError, match="image"):                          # question 1 names image 1: not in the bank yet
        vb.assemble([0, 1])
    vb.add_images((torch.zeros(1, 3, 8), torch.zeros(1, 3, dtype=torch.int64)))
    with pytest.raises(ValueError, match="mode"):
        vb.assemble([0, 1], mode="full")
    with pytest.raises(ValueError, match="mode"):
        vb.assemble([0, 1], mode=["bi"])
    with pytest.raises(ValueError):
        vb.assemble([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # a missing kernel is an error, not a host loop
        vb.assemble([0, 1])
    vb.add_texts(ids, [1, 1])
    with pytest.raises(ValueError, match="add_questions"):
        vb.assemble([0])
