"""Shared definitions of the report-bank tests (no GPU, no package import): plain-numpy statements of what csrc/mv_report.hip computes
-- the counter-based hash and the draws, the masking rule of mv_report_assemble, the row plan of mv_report_plan -- and the case
generator of the sweeps.  Each restatement takes `defect=`: a planted mistake the case set must tell from the rule
(test_report_bank_cases_cpu.py).

The rule (include/medvill.h; the reference's Preprocess4Seq2seq, Downstream_task/report_generation_and_vqa/sc/data_loader.py:340-419):
item d of length len (counting the last [SEP]) lists p = min(n_pred[d], max_pred, len) predictions.  The candidates 0 .. len-1 are
ordered by (word, index); with the coin (top bit of word T) set the first p - 1 of that order are listed and then index len-1, else the
first p.  A listed index t gives (N + 2 + t, original id, 1.0) and holds [MASK] in the input row; the other slots are (0, 0, 0).
"""
import numpy as np

PAD, SEP, MASK = 0, 102, 103
FAMILY_S2S, FAMILY_BAR, FAMILY_1D = 1, 2, 4
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ hash and draws
def hash32(x, k0, k1):
    """csrc/mv_common.h mv_hash32 on 32-bit counters (any shape) -> uint64 array of 32-bit words."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = ((x ^ np.uint64(k0)) * np.uint64(0x9E3779B1)) & _M32
    x ^= x >> np.uint64(15)
    x = ((x ^ np.uint64(k1)) * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(13)
    x ^= x >> np.uint64(16)
    return x


def derive_keys(key, step):
    kk = (int(key) ^ ((int(step) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
    return kk & 0xFFFFFFFF, kk >> 32


def draws(key, step, B, T):
    """uint64 [B, T+1]: word (i, t) = hash32(i (T+1) + t); t < T the shuffle keys, t = T the coin."""
    k0, k1 = derive_keys(key, step)
    return hash32(np.arange(B * (T + 1), dtype=np.uint64), k0, k1).reshape(B, T + 1)


def n_pred_of(length, max_pred=10, mask_prob=0.15):
    """`length` counts the [SEP]; Python's round, as the reference (data_loader.py:346)."""
    return min(max_pred, max(1, int(round((length - 1) * mask_prob))))


# ------------------------------------------------------------------------------------------------ assemble
def chosen_indices(words, length, p, T, defect=None):
    """The listed text indices of one sample, in slot order."""
    w = [int(v) for v in words[:length]]
    if defect == "tie_high":
        order = sorted(range(length), key=lambda t: (w[t], -t))
    else:
        order = sorted(range(length), key=lambda t: (w[t], t))
    coin = (int(words[T]) >> 31) & 1
    if defect == "coin_inverted":
        coin ^= 1
    if coin and p > 0 and defect != "no_sep":
        return order[:p - 1] + [length - 1]
    return order[:p]


def assemble(bank, idx, max_pred, words, family=None, defect=None):
    """bank: dict(txt_ids [n, T], txt_len [n], n_pred [n], img_feats [n, N, F], img_pos [n, N]); idx [B]; words uint [B, T+1]."""
    ids, lens = np.asarray(bank["txt_ids"], np.int64), np.asarray(bank["txt_len"], np.int64)
    n, T = ids.shape
    N = bank["img_pos"].shape[1]
    B = len(idx)
    out = dict(input_txt=np.zeros((B, T), np.int64), segment=np.zeros((B, T), np.int64), desc=np.zeros((B, 3), np.int32),
               feats=np.zeros((B,) + bank["img_feats"].shape[1:], bank["img_feats"].dtype), pos=np.zeros((B, N), np.int64),
               masked_pos=np.zeros((B, max_pred), np.int64), masked_lm_labels=np.zeros((B, max_pred), np.int64),
               masked_weights=np.zeros((B, max_pred), np.float32))
    for i in range(B):
        d = min(max(int(idx[i]), 0), n - 1)
        ln = min(max(int(lens[d]), 1), T)
        p = max(min(int(bank["n_pred"][d]), max_pred, ln), 0)
        out["input_txt"][i] = ids[d]
        for j, t in enumerate(chosen_indices(words[i], ln, p, T, defect)):
            out["masked_pos"][i, j], out["masked_lm_labels"][i, j], out["masked_weights"][i, j] = N + 2 + t, ids[d, t], 1.0
            out["input_txt"][i, t] = MASK
        out["segment"][i, :ln] = 1
        out["desc"][i] = (FAMILY_S2S if family is None else int(family[i]), N + 2, N + 2 + ln)
        out["feats"][i], out["pos"][i] = bank["img_feats"][d], bank["img_pos"][d]
    return out


# ------------------------------------------------------------------------------------------------ plan
def plan(pos, labels, weights, L, V, valid_len=None, defect=None):
    """-> dict(rows, row_ptr, labels, weights, sample, counts = [U, n, bad, 0]) of numpy arrays, as mv_report_plan defines them."""
    pos, labels, weights = np.asarray(pos, np.int64), np.asarray(labels, np.int64), np.asarray(weights, np.float32)
    B, P = pos.shape
    ent, bad = [], 0
    for b in range(B):
        for j in range(P):
            w = weights[b, j]
            if not np.isfinite(w) or w < 0:
                bad += 1
                continue
            if w == 0:
                continue
            hi = L if valid_len is None else min(L, int(valid_len[b]))
            if pos[b, j] <= 0 or pos[b, j] >= hi or labels[b, j] < 0 or labels[b, j] >= V:
                bad += 1
                continue
            ent.append((b * L + int(pos[b, j]), j, int(labels[b, j]), w, b))
    ent.sort(key=lambda e: (e[0], -e[1] if defect == "slot_order" else e[1]))
    if defect == "drop_duplicate":
        seen, kept = {}, []
        for e in ent:
            seen[e[0]] = seen.get(e[0], 0) + 1
            if seen[e[0]] != 2:
                kept.append(e)
        ent = kept
    rows = sorted({e[0] for e in ent})
    row_of = {r: u for u, r in enumerate(rows)}
    row_ptr = np.zeros(len(rows) + 1, np.int32)
    for e in ent:
        row_ptr[row_of[e[0]] + 1] += 1
    return dict(rows=np.array(rows, np.int32), row_ptr=np.cumsum(row_ptr).astype(np.int32),
                labels=np.array([e[2] for e in ent], np.int32), weights=np.array([e[3] for e in ent], np.float32),
                sample=np.array([e[4] for e in ent], np.int32), counts=np.array([len(rows), len(ent), bad, 0], np.int32))


# ------------------------------------------------------------------------------------------------ cases
def make_bank(n_items, T, N, F, seed, max_pred=10, mask_prob=0.15, vocab=3000, lengths=None):
    """A synthetic bank.  Item 0 has len = 1 (only the [SEP]) and item 1 len = T; the rest are drawn.  Token ids avoid 0 and 100..103;
    the features are multiples of 1/8 of magnitude <= 8: exact in f32, bf16 and f16, so a gather is a copy in every encoding."""
    g = np.random.default_rng(seed)
    if lengths is None:
        lengths = g.integers(1, T + 1, n_items)
        lengths[0] = 1
        if n_items > 1:
            lengths[1] = T
    lengths = np.asarray(lengths, np.int64)
    ids = np.zeros((n_items, T), np.int64)
    for d in range(n_items):
        ln = int(lengths[d])
        ids[d, :ln - 1] = g.integers(200, vocab, ln - 1)
        ids[d, ln - 1] = SEP
    feats = (g.integers(-64, 65, (n_items, N, F)) / 8.0).astype(np.float32)
    pos = np.sort(g.integers(0, 256, (n_items, N)), axis=1).astype(np.int64)
    n_pred = np.array([n_pred_of(int(ln), max_pred, mask_prob) for ln in lengths], np.int32)
    return dict(txt_ids=ids, txt_len=lengths.astype(np.int32), n_pred=n_pred, img_feats=feats, img_pos=pos)


def injected_draws(B, T, seed, kind="random"):
    """uint64 [B, T+1] words given by the caller.  "equal": every shuffle key the same (the order is the index order); "descending":
    keys fall with the index (the order is reversed); coins alternate between samples in both."""
    g = np.random.default_rng(seed)
    w = g.integers(0, 1 << 32, (B, T + 1), dtype=np.uint64)
    if kind == "equal":
        w[:, :T] = 12345
    elif kind == "descending":
        w[:, :T] = (1000000 - np.arange(T, dtype=np.uint64))[None, :]
    if kind != "random":
        w[:, T] = np.where(np.arange(B) % 2 == 0, 0x80000000, 0x7FFFFFFF).astype(np.uint64)
    return w


# (T, B, max_pred, N, F, dtype name, draws kind or "hash"): every value the sweep names appears; B = 257 and F = 2048 meet once each
# per dtype family, and the 64 KiB copy chunks (N F bytes > 65536) are crossed at N = 16, F = 2048
SWEEP = [
    (2, 1, 1, 1, 8, "f32", "hash"),
    (3, 3, 3, 1, 8, "bf16", "random"),
    (17, 3, 10, 16, 8, "f16", "equal"),
    (17, 64, 64, 1, 8, "f32", "descending"),
    (64, 64, 10, 16, 8, "bf16", "hash"),
    (65, 3, 64, 1, 2048, "f16", "hash"),
    (65, 257, 3, 1, 8, "f32", "random"),
    (253, 64, 10, 16, 2048, "bf16", "hash"),
    (253, 3, 64, 16, 2048, "f32", "equal"),
    (253, 257, 10, 1, 8, "f16", "descending"),
    (3, 1, 64, 16, 2048, "f16", "random"),
    (64, 3, 1, 16, 8, "f32", "hash"),
]
# the guard elements in front of every output of a sweep case; 3 puts the feature rows off a 16-byte boundary, which takes the copy's
# element-by-element path ("odd-guard" cases)
GUARD, GUARD_ODD = 16, 3
# further cases of the assembly sweep, chosen for the feature copy (csrc/mv_bank.h): whole vectors off their alignment; N F = 20500 in
# f32 -- two chunks, the last one unrolled round and a 5-vector remainder; 36936 in f16 -- a last chunk of 521 vectors, no whole round.
# test_bank_cases_cpu.py shows which branches of the copy SWEEP + COPY_CASES reach.
COPY_CASES = [
    (17, 3, 3, 1, 8, "bf16", "odd-guard"),
    (17, 3, 3, 5, 4100, "f32", "hash"),
    (17, 3, 3, 9, 4104, "f16", "hash"),
]


def plan_case(kind, B=5, P=6, L=40, V=300, seed=0):
    """Named list cases of the plan tests: -> (pos, labels, weights, valid_len or None)."""
    g = np.random.default_rng(seed)
    pos = g.integers(1, L, (B, P)).astype(np.int64)
    lab = g.integers(1, V, (B, P)).astype(np.int64)
    w = np.ones((B, P), np.float32)
    vl = None
    if kind == "duplicates":                          # one position two and three times, equal and different labels
        pos[0, :3], lab[0, :3] = 7, (11, 11, 12)
        if B > 1 and P >= 5:
            pos[1, 1], pos[1, 4], lab[1, 1], lab[1, 4] = 9, 9, 5, 5
    elif kind == "zero_weight":
        w[:, ::2] = 0.0
        pos[0, 0], lab[0, 0] = 0, 0                   # the reference's padding: (0, 0, 0)
    elif kind == "label0":
        lab[:, 0] = 0
    elif kind == "fractional":
        w[:] = g.integers(1, 9, (B, P)) / 8.0
    elif kind == "all_zero":
        w[:] = 0.0
        pos[:], lab[:] = 0, 0
    elif kind == "valid_len":
        vl = np.full(B, L, np.int32)
        pos = np.minimum(pos, L - 2)
    elif kind != "plain":
        raise ValueError(kind)
    return pos, lab, w, vl


BAD_KINDS = ("position0", "negative_position", "past_sequence", "past_valid_len", "label_negative", "label_past_vocab", "negative_weight",
             "nan_weight", "inf_weight")


def spoil(kind, pos, lab, w, vl, L, V, b=1, j=2):
    """One bad entry of the named kind at (b, j) (in place); -> valid_len to use."""
    if kind == "position0":
        pos[b, j] = 0
    elif kind == "negative_position":
        pos[b, j] = -3
    elif kind == "past_sequence":
        pos[b, j] = L
    elif kind == "past_valid_len":
        vl = np.full(pos.shape[0], L, np.int32) if vl is None else vl
        vl[b] = L - 5
        pos[b] = np.minimum(pos[b], L - 6)            # the sample's other entries stay inside
        pos[b, j] = L - 5
    elif kind == "label_negative":
        lab[b, j] = -1
    elif kind == "label_past_vocab":
        lab[b, j] = V
    elif kind == "negative_weight":
        w[b, j] = -0.5
    elif kind == "nan_weight":
        w[b, j] = np.nan
    elif kind == "inf_weight":
        w[b, j] = np.inf
    else:
        raise ValueError(kind)
    return vl
