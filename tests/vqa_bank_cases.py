"""Shared definitions of the VQA-bank tests (no GPU, no package import): plain-numpy statements of what csrc/mv_vqa_bank.hip computes --
mv_vqa_assemble's batch and mv_vqa_score's scores and counters --, of the reference's target construction and type mapping, and the
case generator of the sweeps; the launcher's chunk plan is the shared one of tests/bank_cases.py.  Each
restatement takes `defect=`: a planted mistake the comparison of the sweep must tell from the rule (test_vqa_bank_cases_cpu.py).

The rule (include/medvill.h).  The reference's VQA-RAD loader (Downstream_task/report_generation_and_vqa/sc/data_loader.py:236-273)
turns a question's answer['labels'] / answer['scores'] into a dense target of zeros with target[label] = score, by scatter_ (:269-271):
a label listed twice keeps its LATER score.  Preprocess4Seq2seq lays a question out as tokens + [SEP] + [PAD]... with segment 1 over the
tokens and the [SEP] (:342-348, :392) and masks nothing (:378-381); the answer type strings map to 0 / 1 (:434-437).  The score of a
prediction is the target's value at the predicted column (pytorch_pretrained_bert/model.py:1007-1012, 1023)."""
import os

import numpy as np

import bank_cases
from bank_cases import ALL_BRANCHES, ITEMSIZE, launch_plan          # noqa: F401  (the plan is the three bank kernels' one)

PAD, SEP = 0, 102
FAMILY_S2S, FAMILY_BAR, FAMILY_1D = 1, 2, 4
HIP_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-modality-self-supervision_amd", "csrc",
                          "mv_vqa_bank.hip")


# ------------------------------------------------------------------------------------------------ the reference, restated
def answer_type(t):
    """data_loader.py:434-437: the strings with their trailing-space variants; an integer 0 / 1 passes; anything else is 2."""
    if isinstance(t, str):
        return {"CLOSED": 0, "CLOSED ": 0, "OPEN": 1, "OPEN ": 1}.get(t, 2)
    return int(t) if t in (0, 1) else 2


def reference_target(labels, scores, A):
    """data_loader.py:253-271: zeros(A), then the (label, score) pairs in their order; None or an empty list leaves the zeros."""
    t = np.zeros(A, np.float32)
    if labels is not None:
        for l, s in zip(labels, scores):
            t[int(l)] = np.float32(s)
    return t


# ------------------------------------------------------------------------------------------------ mv_vqa_assemble
def clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def assemble(bank, idx, A, family=None, defect=None):
    """bank: dict(txt_ids [n, T], txt_len [n], q_img [n], ans_ptr [n+1], ans_label [nnz], ans_score [nnz], ans_type [n], group [n],
    img_feats [n_img, N, F], img_pos [n_img, N]); idx [B] -> dict(input_txt, segment, desc, feats, pos, target, ans_type)."""
    ids = np.asarray(bank["txt_ids"], np.int64)
    n, T = ids.shape
    n_img, N = bank["img_pos"].shape
    nnz = len(bank["ans_label"])
    B = len(idx)
    out = dict(input_txt=np.zeros((B, T), np.int64), segment=np.zeros((B, T), np.int64), desc=np.zeros((B, 3), np.int32),
               feats=np.zeros((B,) + bank["img_feats"].shape[1:], bank["img_feats"].dtype), pos=np.zeros((B, N), np.int64),
               target=np.zeros((B, A), np.float32), ans_type=np.zeros(B, np.int32))
    for i in range(B):
        d = clamp(idx[i], 0, n - 1)
        m = clamp(d if defect == "image_from_idx" else bank["q_img"][d], 0, n_img - 1)
        ln = clamp(bank["txt_len"][d], 1, T)
        if defect == "len_off_by_one":
            ln -= 1
        out["input_txt"][i] = ids[d]
        out["segment"][i, :] = 1 if defect == "segment_ones" else 0
        out["segment"][i, :ln] = 1
        out["desc"][i] = (FAMILY_1D if family is None else int(family[i]), N + 2, N + 2 + ln)
        out["feats"][i], out["pos"][i] = bank["img_feats"][m], bank["img_pos"][m]
        e0 = clamp(bank["ans_ptr"][d], 0, nnz)
        e1 = clamp(bank["ans_ptr"][d + 1], e0, nnz)
        written = set()
        for e in range(e0, e1):
            l = int(bank["ans_label"][e])
            if not 0 <= l < A or (defect == "first_duplicate" and l in written):
                continue
            out["target"][i, l] = bank["ans_score"][e]
            written.add(l)
        out["ans_type"][i] = bank["ans_type"][d]
    return out


# ------------------------------------------------------------------------------------------------ mv_vqa_score
def fx(s, defect=None):
    """32.32 fixed point of an f32 score widened to f64, rounded to nearest even."""
    x = np.float64(np.float32(s)) * 4294967296.0
    return int(np.trunc(x)) if defect == "fx_truncated" else int(np.rint(x))


def score(bank, pred, idx, G, use_group=True, counters=None, defect=None):
    """-> (score f32 [B], counters int64 [G, 3, 2] = `counters` plus this batch's {fx(score), 1} by (group, type slot))."""
    n, nnz = len(bank["txt_len"]), len(bank["ans_label"])
    cnt = np.zeros((G, 3, 2), np.int64) if counters is None else np.array(counters, np.int64).reshape(G, 3, 2)
    sc = np.zeros(len(idx), np.float32)
    for i in range(len(idx)):
        d = clamp(idx[i], 0, n - 1)
        e0 = clamp(bank["ans_ptr"][d], 0, nnz)
        e1 = clamp(bank["ans_ptr"][d + 1], e0, nnz)
        for e in range(e0, e1):
            if int(bank["ans_label"][e]) == int(pred[i]):
                sc[i] = bank["ans_score"][e]                      # the last entry of the label
        ty = int(bank["ans_type"][d])
        slot = 0 if ty == 0 else (1 if ty == 1 else 2)
        if defect == "slot_swapped":
            slot = (1, 0, 2)[slot]
        g = clamp(bank["group"][d], 0, G - 1) if use_group else 0
        cnt[g, slot, 0] += fx(sc[i], defect)
        cnt[g, slot, 1] += 1
    return sc, cnt


def metrics(counters):
    """The six numbers of an evaluation from the integer counters, in f64: acc over every sample, the splits over their own; nan for
    an empty split."""
    c = np.asarray(counters, np.int64).reshape(-1, 3, 2)

    def ratio(a, b):
        return float(np.float64(int(a)) / np.float64(4294967296.0) / np.float64(int(b))) if b else float("nan")

    def six(g):
        f, k = g[:, :, 0].sum(0), g[:, :, 1].sum(0)
        return dict(acc=ratio(f.sum(), k.sum()), closed_acc=ratio(f[0], k[0]), open_acc=ratio(f[1], k[1]), n=int(k.sum()),
                    closed_n=int(k[0]), open_n=int(k[1]))

    out = six(c)
    out["by_group"] = {g: six(c[g:g + 1]) for g in range(c.shape[0]) if c[g, :, 1].sum()}
    return out


# ------------------------------------------------------------------------------------------------ the launcher's plan
def source_constants():
    """The constants of the shared gather (csrc/mv_bank.h) and of the kernel file."""
    return bank_cases.source_constants(bank_cases.BANK_HEADER, HIP_SOURCE)


# ------------------------------------------------------------------------------------------------ cases
# scores: the reference's soft scores, plus values with bits below 2^-32 (there fx rounds, and truncation differs) and a negative one
SCORES = np.array([1.0, 0.6, 0.3, 0.9, 1e-6, 7.3e-8, 3.1e-9, -0.25], np.float32)


def make_bank(n_q, n_img, T, N, F, A, seed, q_img_outside=False, vocab=3000):
    """A synthetic question bank.  Question 0: len = 1 (only the [SEP]) and no answers; question 1: len = T and one answer, label A - 1;
    question 2: one label listed twice with different scores (and, when A allows, another in between); questions 2, 3 and 4 share image
    0; the rest are drawn (0 .. 4 answers, labels possibly repeated).  ans_type cycles 0 / 1 / 2; group leaves group 5 empty.
    q_img_outside: questions 3 and 4 name images n_img + 2 and -1 (the kernel clamps them).  Token ids avoid 0 and 100..103; the
    features are multiples of 1/8 of magnitude <= 8: exact in f32, bf16 and f16, so a gather is a copy in every encoding."""
    g = np.random.default_rng(seed)
    lengths = g.integers(1, T + 1, n_q)
    lengths[0] = 1
    if n_q > 1:
        lengths[1] = T
    ids = np.zeros((n_q, T), np.int64)
    for d in range(n_q):
        ln = int(lengths[d])
        ids[d, :ln - 1] = g.integers(200, vocab, ln - 1)
        ids[d, ln - 1] = SEP
    q_img = g.integers(0, n_img, n_q)
    q_img[2:5] = 0
    if q_img_outside and n_q > 4:
        q_img[3], q_img[4] = n_img + 2, -1
    labels, scores = [], []
    for d in range(n_q):
        if d == 0:
            l, s = [], []
        elif d == 1:
            l, s = [A - 1], [float(SCORES[4])]                   # a score with bits below 2^-32
        elif d == 2:
            a = int(g.integers(0, A))
            l, s = ([a, (a + 1) % A, a] if A > 1 else [a, a]), ([0.3, 1e-6, 0.9] if A > 1 else [0.3, 0.9])
        else:
            k = int(g.integers(0, 5))
            l = g.integers(0, A, k).tolist()
            s = g.choice(SCORES, k).tolist()
        labels.append(l)
        scores.append(s)
    ptr = np.zeros(n_q + 1, np.int32)
    ptr[1:] = np.cumsum([len(l) for l in labels])
    group = g.choice([0, 1, 2, 3, 4, 6, 7], n_q)
    return dict(txt_ids=ids, txt_len=lengths.astype(np.int32), q_img=q_img.astype(np.int32), ans_ptr=ptr,
                ans_label=np.array([x for l in labels for x in l], np.int32), ans_score=np.array([x for s in scores for x in s], np.float32),
                ans_type=(np.arange(n_q) % 3).astype(np.int32), group=group.astype(np.int32), labels=labels, scores=scores,
                img_feats=(g.integers(-64, 65, (n_img, N, F), dtype=np.int8) / np.float32(8.0)).astype(np.float32),
                img_pos=np.sort(g.integers(0, 256, (n_img, N)), axis=1).astype(np.int64))


def batch_idx(bank, B, seed, clamped=True):
    """int32 [B]: questions 0 (no answers, len 1), 1 (len T) and 2 (the duplicate) first as far as B allows, a repeated question, and
    -- clamped -- an index below 0 and one past the bank."""
    n = len(bank["txt_len"])
    g = np.random.default_rng(seed)
    idx = g.integers(0, n, B).astype(np.int32)
    idx[:min(B, 3)] = [0, 1, 2][:min(B, 3)]
    if B == 1:
        idx[0] = n + 2 if clamped else 2
    if B >= 6:
        idx[3] = idx[2]                                           # side by side, the same question
        if clamped:
            idx[4], idx[5] = -4, n
    return idx


def batch_pred(bank, idx, A, seed):
    """int64 [B] answer columns: by turns the question's last listed label, its first (the duplicated one of question 2), a column it
    does not list, and A - 1."""
    n = len(bank["txt_len"])
    g = np.random.default_rng(seed)
    pred = np.zeros(len(idx), np.int64)
    for i, q in enumerate(idx):
        d = clamp(q, 0, n - 1)
        mine = bank["ans_label"][bank["ans_ptr"][d]:bank["ans_ptr"][d + 1]].tolist()
        kind = (i + 2) % 4                                        # sample 1 (question 1): A - 1; sample 2 (question 2): the duplicate
        if kind == 0 and mine:
            pred[i] = mine[-1]
        elif kind == 1 and mine:
            pred[i] = mine[0]
        elif kind == 2:
            free = [a for a in range(A) if a not in mine]
            pred[i] = free[int(g.integers(0, len(free)))] if free else 0
        else:
            pred[i] = A - 1
    return pred


# (B, A, T, N, F, dtype name, family: None or "per", groups: None or 8, guard elements in front of every output).  A guard of 3 puts
# the feature rows off a 16-byte boundary.  test_vqa_bank_cases_cpu.py shows that the set reaches every branch of the launcher.
GUARD, GUARD_ODD = 16, 3
SWEEP = [
    (1, 1, 2, 1, 7, "f32", None, None, GUARD),                    # a row that is no whole vector: element by element
    (3, 17, 46, 3, 11, "bf16", "per", 8, GUARD),
    (64, 458, 46, 1, 8, "f16", None, 8, GUARD),                   # one vector per row
    (3, 458, 1024, 16, 2048, "f32", "per", None, GUARD),          # two full chunks of unrolled rounds only
    (6, 17, 2, 5, 4100, "f32", None, 8, GUARD),                   # the last chunk: one round and a 5-vector remainder
    (64, 458, 46, 16, 2048, "bf16", "per", 8, GUARD),             # the flagship row: one full chunk
    (6, 17, 46, 9, 4104, "f16", None, None, GUARD),               # the last chunk: 521 vectors, no whole round
    (3, 17, 46, 1, 8, "bf16", "per", 8, GUARD_ODD),               # whole vectors off their alignment
    (6, 458, 46, 2, 8, "f32", None, None, GUARD_ODD),
    (1, 17, 2, 1, 16777244, "f32", None, 8, GUARD),               # more chunks than the grid's cap: larger chunks
]


def sweep_bank(case):
    B, A, T, N, F, dtn, fam, grp, guard = case
    n_img = 2 if N * F > 1 << 20 else 3
    return make_bank(max(6, min(B, 20)), n_img, T, N, F, A, seed=B * 1000 + T + A, q_img_outside=True)
