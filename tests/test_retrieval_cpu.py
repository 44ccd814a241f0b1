"""Retrieval without a GPU: the numpy definitions of tests/retrieval_cases.py against the upstream project's own metric functions (recorded
in tests/golden/retrieval_metrics.npz by tools/gen_retrieval_golden.py), the sampler definition against a replay of the upstream
procedure, and the host-only logic of RetrievalBank / evaluate."""
import os

import numpy as np
import pytest
import torch

import medvill_amd as mv
from medvill_amd import retrieval as R
from medvill_amd.data import RetrievalBank, check_pairs

import retrieval_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval_metrics.npz")


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_numpy_metrics_equal_the_upstream_functions(case):
    z = np.load(GOLDEN)
    C = int(z[f"{case}_C"])
    sims, labels, ids = z[f"{case}_sims"], z[f"{case}_labels"], z[f"{case}_ids"]
    assert sims.dtype == np.float32 and all(len(set(g.tolist())) == C for g in sims.reshape(-1, C))      # distinct: no tie rule involved
    assert (labels.reshape(-1, C).sum(axis=1) > 0).all()
    m = RC.metrics(sims, labels, C)
    assert m["rank"].tolist() == z[f"{case}_ranks"].tolist()
    assert [[int(ids[j]), r] for j, r in m["aligned"]] == z[f"{case}_aligned"].tolist()
    assert [round(v, 3) for v in m["recall"]] == z[f"{case}_recall"].tolist()         # upstream rounds where it builds the dictionaries
    assert [round(v, 3) for v in m["precision"]] == z[f"{case}_precision"].tolist()
    assert abs(m["mrr"] - float(z[f"{case}_mrr"])) <= 1e-15
    # the integer sums the kernel keeps, and what summarize() makes of them, say the same
    pos = RC.positions(sims, C)
    s = R.summarize(RC.counters(pos, labels, C), RC.KS)
    G = labels.size // C
    for q, k in enumerate(RC.KS):
        assert s["hits"][f"R@{k}"] == m["hits"][q]
        assert abs(s["recall"][f"R@{k}"] - m["recall"][q]) <= 2.0 ** -32 and abs(s["precision"][f"R@{k}"] - m["precision"][q]) <= 1e-15
    assert abs(s["mrr_score"] - m["mrr"]) <= 2.0 ** -32 and s["groups"] == G and s["groups_without_aligned"] == 0
    assert R.aligned_list(pos, labels, C, ids=ids) == z[f"{case}_aligned"].tolist()


def test_tie_rule_nan_and_groups_without_an_aligned_candidate():
    p = np.float32([0.5, 0.5, 0.9, np.nan, 0.5, 0.0, np.nan])
    assert RC.group_order(p).tolist() == [2, 4, 1, 0, 5, 6, 3]                  # ties: higher index first; NaN last, again higher first
    assert RC.positions(p, 7).tolist() == [3, 2, 0, 6, 1, 4, 5]
    assert RC.group_order(np.float32([0.25] * 5)).tolist() == [4, 3, 2, 1, 0]   # = np.argsort(kind="stable")[::-1]
    assert np.argsort(np.float32([0.25] * 5), kind="stable")[::-1].tolist() == [4, 3, 2, 1, 0]
    lab = np.int32([0] * 7)
    pos = RC.positions(p, 7)
    assert RC.group_ranks(pos, lab, 7).tolist() == [7]
    c = RC.counters(pos, lab, 7)
    assert c[0] == 1 and c[1] == 1 and c[2] == RC.fx(1 / 8) and c[4:7] == [0, 0, 1] and c[12:15] == [0, 0, 0] and c[20:23] == [0, 0, 0]
    s = R.summarize(c, RC.KS)
    assert s["hits"] == {"R@1": 0.0, "R@5": 0.0, "R@10": 1.0} and np.isnan(s["recall"]["R@1"]) and s["mrr_score"] == 0.125
    assert R.aligned_list(pos, lab, 7) == [[3, 7]]                              # the last candidate in the order, as upstream's loop leaves it
    lab2 = np.int32([1, 0, 0, 0, 1, 0, 0])
    c2 = RC.counters(pos, lab2, 7)                                              # k = 10 > C takes the whole group
    assert c2[4:7] == [0, 1, 1] and c2[20:23] == [0, 2, 2] and c2[12:15] == [0, RC.fx(1.0), RC.fx(1.0)] and R.aligned_list(pos, lab2, 7) == [[4, 1]]


@pytest.mark.parametrize("name", sorted(RC.sampler_cases()))
def test_sampler_definition_equals_a_replay_of_the_upstream_procedure(name):
    c = RC.sampler_cases()[name]
    pairs, labels = RC.sample_negatives(c["idx"], c["n"], c["draws"], c["class_id"])
    rp, rl = RC.replay_negatives(c["idx"], c["n"], c["draws"], c["class_id"])
    assert pairs.tolist() == rp.tolist() and labels.tolist() == rl.tolist()
    B, n = len(c["idx"]), c["n"]
    neg = pairs[B:]
    assert pairs[:B].tolist() == [[d, d] for d in c["idx"]]
    assert ((neg >= 0) & (neg < n)).all() and (neg[:, 0] != neg[:, 1]).all()                    # never the sample itself
    assert ((neg[:, 0] == c["idx"]) ^ (neg[:, 1] == c["idx"])).all()                            # exactly one side is replaced
    if name.startswith("plain"):
        # d = 0 / n-1 with w0 = 0 / 2^32-1: the first and the last of the other indices; the coin picks the side
        assert pairs[B:B + 8].tolist() == [[0, 1], [n - 1, 0], [0, n - 1], [n - 1, n - 2], [1, 0], [0, n - 1], [n - 1, 0], [n - 2, n - 1]]
    if name.startswith("one_other_class"):
        other = np.where(neg[:, 0] == c["idx"], neg[:, 1], neg[:, 0])
        found = c["class_id"][other] != c["class_id"][np.asarray(c["idx"])]
        assert found.sum() >= 1                                                                 # (n = 3: one try in two finds it)
        assert all(int(o) == n // 2 for o, f, d in zip(other, found, c["idx"]) if f and d != n // 2)       # the one item of the other class
    if name.startswith("all_one_class"):                                                        # 300 draws used up: the last one is kept
        last, _ = RC.sample_negatives(c["idx"], n, c["draws"][:, -1:, :], None)
        assert pairs.tolist() == last.tolist()


def test_assembled_batch_definition():
    ids, lens, feats, pos = RC.make_banks(5, 4, 3, 5, 8, seed=1)
    b = RC.assemble(ids, lens, feats, pos, [(0, 4), (3, 0), (3, 0), (1, 2)])
    assert b["input_txt"].shape == (4, 6) and (b["segment"] == 1).all() and b["n_ids"].tolist() == [6, 1, 1, int(lens[2])]
    want = mv.data.MaskDesc.make("1d", 3, 5, b["n_ids"])
    assert torch.equal(torch.from_numpy(b["desc"]), want.desc) and want.L == 3 + 5 + 3
    assert (b["input_txt"][1] == [102, 0, 0, 0, 0, 0]).all() and b["input_txt"][0, 5] == 102
    assert np.array_equal(b["feats"][1], b["feats"][2]) and np.array_equal(b["feats"][3], feats[1])


def test_group_plan_and_pair_checks():
    assert R.group_plan(12, 6, 5) == (2, [(0, 5), (5, 10), (10, 12)])
    assert R.group_plan(6, 6, 100) == (1, [(0, 6)])
    for bad in ((13, 6, 5), (0, 6, 5), (12, 0, 5), (12, 6, 0), (5, 6, 5)):
        with pytest.raises(ValueError):
            R.group_plan(*bad)
    assert check_pairs([[0, 1], [2, 0]], 3, 2).dtype == torch.int32
    for bad, err in (([[3, 0]], IndexError), ([[0, 2]], IndexError), ([[-1, 0]], IndexError), ([[0, -1]], IndexError), ([[0, 1, 2]], ValueError),
                     ([], ValueError), ([[0.5, 1.0]], ValueError)):
        with pytest.raises(err):
            check_pairs(bad, 3, 2)


def test_retrieval_bank_host_logic():
    ids, lens, feats, pos = RC.make_banks(5, 4, 3, 5, 8, seed=2)
    bank = RetrievalBank(None, device="cpu", feat_dtype=torch.float32)
    with pytest.raises(RuntimeError):
        bank.assemble([[0, 0]])
    bank.add_texts(torch.from_numpy(ids[:2]), lens[:2]).add_texts(ids[2:], torch.from_numpy(lens[2:]))
    bank.add_images((torch.from_numpy(feats), torch.from_numpy(pos)))
    assert bank.n_texts == 5 and bank.n_images == 4 and bank.img_feats.dtype == torch.float32
    pairs = check_pairs([(0, 4), (3, 0), (1, 2)], bank.n_images, bank.n_texts)
    d = bank.host_descriptors(pairs)
    assert torch.equal(d, torch.from_numpy(RC.assemble(ids, lens, feats, pos, pairs.numpy())["desc"]))
    assert torch.equal(d, mv.data.MaskDesc.make("1d", 3, 5, lens[[4, 0, 2]]).desc)
    with pytest.raises(ValueError):
        bank.add_texts(ids[:1], [0])                       # a length counts the [SEP]
    with pytest.raises(ValueError):
        bank.add_texts(ids[:1], [7])
    with pytest.raises(ValueError):
        bank.add_texts(ids[:1, :4], [2])                   # another S
    with pytest.raises(ValueError):
        bank.add_images((torch.zeros(1, 2, 8), torch.zeros(1, 2, dtype=torch.int64)))
    with pytest.raises(IndexError):
        bank.assemble([[4, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.assemble([[0, 0]])                            # the assembly itself is a HIP kernel


def test_evaluate_rejects_a_pair_count_that_is_no_multiple_of_the_group_size():
    m = R.CXRBertForRetrieval.__new__(R.CXRBertForRetrieval)
    torch.nn.Module.__init__(m)
    m.bert = type("B", (), {"engine": type("E", (), {"device": torch.device("cpu")})()})()
    with pytest.raises(ValueError, match="whole groups"):
        R.CXRBertForRetrieval.evaluate(m, None, [[0, 0]] * 7, [1] * 7, group_size=6)
