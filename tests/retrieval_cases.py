"""Shared definitions of the retrieval tests (no GPU): plain-numpy statements of what csrc/mv_retrieval.hip computes -- the three ranking
metrics with the tie rule, the negative sampler on given draws, the assembled pair batch -- and the case lists the CPU and GPU tests run.

Order within a group: descending p, exact ties by the HIGHER candidate index first, NaN after every number (what reversing a stable
ascending sort gives for numbers; include/medvill.h, mv_rank_groups)."""
import numpy as np

KS = (1, 5, 10)
GROUP_SIZES = (1, 2, 7, 64, 65, 257, 1000)
GROUP_COUNTS = (1, 3, 300)
MAX_DRAWS = 300
NCOUNT = 28
FAMILY_1D = 4


# ---------------------------------------------------------------------------------------------------- metrics
def group_order(p):
    """candidate indices of one group, best first"""
    p = np.asarray(p, dtype=np.float32)
    key = np.where(np.isnan(p), np.float32(-1.0), p)
    return np.lexsort((-np.arange(p.size), -key.astype(np.float64)))


def positions(p, C):
    """pos [G*C]: the number of candidates of the same group ahead of each candidate"""
    p = np.asarray(p, dtype=np.float32).reshape(-1, C)
    pos = np.empty(p.shape, dtype=np.int32)
    for g in range(p.shape[0]):
        pos[g, group_order(p[g])] = np.arange(C, dtype=np.int32)
    return pos.reshape(-1)


def group_ranks(pos, labels, C):
    """rank [G]: the least pos among aligned candidates, C when none is aligned"""
    pos, lab = np.asarray(pos).reshape(-1, C), np.asarray(labels).reshape(-1, C)
    return np.where(lab == 1, pos, C).min(axis=1).astype(np.int32)


def fx(x):
    """32.32 fixed point of the f64 value, rounded to nearest even (np.rint)"""
    return int(np.rint(np.ldexp(np.float64(x), 32)))


def counters(pos, labels, C, ks=KS):
    """the 28 integer sums of mv_rank_groups (include/medvill.h)"""
    pos, lab = np.asarray(pos).reshape(-1, C), np.asarray(labels).reshape(-1, C)
    rank = group_ranks(pos, lab, C)
    c = [0] * NCOUNT
    for g in range(pos.shape[0]):
        al = lab[g] == 1
        total = int(al.sum())
        c[0] += 1
        c[1] += int(total == 0)
        c[2] += fx(np.float64(1.0) / np.float64(int(rank[g]) + 1))
        for q, k in enumerate(ks):
            top = int((al & (pos[g] < k)).sum())
            c[4 + q] += int(rank[g] < k)
            if total > 0:
                c[12 + q] += fx(np.float64(top) / np.float64(total))
            c[20 + q] += top
    return c


def metrics(p, labels, C, ks=KS):
    """Hit@k, recall@k, precision@k and MRR in plain f64, from the order above (the reference's compute_ranks / compute_recall_precision /
    compute_mrr on scores without ties): dict(rank [G], hits, recall, precision: [per k], mrr, aligned: [[candidate, rank]])."""
    lab = np.asarray(labels).reshape(-1, C)
    pos = positions(p, C).reshape(-1, C)
    rank = group_ranks(pos, lab, C)
    hits = [float(np.mean(rank < k)) for k in ks]
    recall, precision = [], []
    for k in ks:
        top = ((lab == 1) & (pos < k)).sum(axis=1).astype(np.float64)
        tot = (lab == 1).sum(axis=1).astype(np.float64)
        has = tot > 0
        recall.append(float(np.mean(top[has] / tot[has])) if has.any() else float("nan"))
        precision.append(float(np.mean(top / k)))
    aligned = []
    for g in range(lab.shape[0]):
        al = np.flatnonzero(lab[g] == 1)
        j = int(al[np.argmin(pos[g][al])]) if al.size else int(np.argmax(pos[g]))
        aligned.append([g * C + j, int(rank[g])])
    return dict(rank=rank, hits=hits, recall=recall, precision=precision, mrr=float(np.mean(1.0 / (rank.astype(np.float64) + 1.0))),
                aligned=aligned)


def _labels(G, C, rng, pattern=None):
    """groups cycle through one / several / all / no aligned candidate (`pattern` forces one of them)"""
    lab = np.zeros((G, C), dtype=np.int32)
    for g in range(G):
        kind = pattern or ("one", "several", "all", "none")[g % 4]
        if kind == "one":
            lab[g, rng.integers(0, C)] = 1
        elif kind == "several":
            lab[g, rng.choice(C, size=max(1, min(C, 3 + C // 16)), replace=False)] = 1
        elif kind == "all":
            lab[g, :] = 1
    return lab.reshape(-1)


def rank_cases():
    """name -> dict(G, C, logits f32 [G*C, 2], labels int32 [G*C])"""
    out = {}
    for C in GROUP_SIZES:
        for G in GROUP_COUNTS:
            rng = np.random.default_rng(1000 * C + G)
            out[f"C{C}_G{G}"] = dict(G=G, C=C, logits=rng.standard_normal((G * C, 2)).astype(np.float32) * 2, labels=_labels(G, C, rng))
    rng = np.random.default_rng(7)
    out["none_aligned_G1"] = dict(G=1, C=7, logits=rng.standard_normal((7, 2)).astype(np.float32), labels=_labels(1, 7, rng, "none"))
    for C in (7, 65, 257):                                   # all scores equal: the order is the tie rule alone
        out[f"all_equal_C{C}"] = dict(G=3, C=C, logits=np.tile(np.float32([0.25, -0.5]), (3 * C, 1)), labels=_labels(3, C, rng))
    for C in (7, 300):                                       # logits of +-40: p is exactly 1.0 for many candidates, tiny for the others
        lg = np.where(rng.random((4 * C, 1)) < 0.5, np.float32([-40.0, 40.0]), np.float32([40.0, -40.0])).astype(np.float32)
        lg[::5] = rng.standard_normal((lg[::5].shape[0], 2)).astype(np.float32)
        out[f"saturated_C{C}"] = dict(G=4, C=C, logits=lg, labels=_labels(4, C, rng))
    for C in (7, 257):                                       # one NaN logit (in an aligned candidate of group 1)
        lg = rng.standard_normal((3 * C, 2)).astype(np.float32)
        lab = _labels(3, C, rng, "several")
        j = C + int(np.flatnonzero(lab[C:2 * C] == 1)[0])
        lg[j, 0] = np.nan
        out[f"nan_C{C}"] = dict(G=3, C=C, logits=lg, labels=lab)
    return out


# ---------------------------------------------------------------------------------------------------- sampler
def sample_negatives(idx, n, draws, class_id=None):
    """The sampler on given draws (uint [B, D, 2] = {w0, w1} of attempt t): -> (pairs int32 [2B, 2], labels int32 [2B])."""
    idx = np.asarray(idx, dtype=np.int64)
    draws = np.asarray(draws, dtype=np.uint64).reshape(idx.size, -1, 2)
    B, D = idx.size, draws.shape[1]
    pairs = np.empty((2 * B, 2), dtype=np.int32)
    tries = min(D, MAX_DRAWS) if class_id is not None else 1
    for i, d in enumerate(idx.tolist()):
        for t in range(tries):
            w0, w1 = int(draws[i, t, 0]), int(draws[i, t, 1])
            r = (w0 * (n - 1)) >> 32
            other = r + (1 if r >= d else 0)
            if class_id is None or class_id[other] != class_id[d]:
                break
        pairs[i] = (d, d)
        pairs[B + i] = (other, d) if (w1 >> 31) else (d, other)
    return pairs, np.concatenate([np.ones(B, np.int32), np.zeros(B, np.int32)])


def replay_negatives(idx, n, draws, class_id=None):
    """The reference's procedure replayed on the same words (CXR_Retrieval_Dataset.__getitem__ / get_random_line): the list of the other
    indices, a choice from it by position r, then the coin; label_conditioned: up to 300 rounds until the classes differ."""
    idx = [int(v) for v in idx]
    draws = np.asarray(draws, dtype=np.uint64).reshape(len(idx), -1, 2)
    pos, neg = [], []
    for i, d in enumerate(idx):
        others = list(range(0, d)) + list(range(d + 1, n))
        rounds = min(draws.shape[1], MAX_DRAWS) if class_id is not None else 1
        for t in range(rounds):
            w0, w1 = int(draws[i, t, 0]), int(draws[i, t, 1])
            rand = others[(w0 * len(others)) // 2 ** 32]
            coin_heads = w1 >= 2 ** 31
            if class_id is None or class_id[rand] != class_id[d]:
                break
        pos.append((d, d))
        neg.append((rand, d) if coin_heads else (d, rand))
    return np.array(pos + neg, dtype=np.int32), np.array([1] * len(idx) + [0] * len(idx), dtype=np.int32)


def sampler_cases():
    """name -> dict(n, idx, draws uint64 [B, D, 2], class_id or None)"""
    out = {}
    hi = 2 ** 32 - 1
    for n in (2, 3, 1000):
        rng = np.random.default_rng(n)
        idx = [0, n - 1, 0, n - 1, 0, n - 1, 0, n - 1] + rng.integers(0, n, 9).tolist()
        w0 = [0, 0, hi, hi, 0, 0, hi, hi] + rng.integers(0, 2 ** 32, 9).tolist()
        w1 = [0, 0, 0, 0, hi, hi, hi, hi] + rng.integers(0, 2 ** 32, 9).tolist()
        out[f"plain_n{n}"] = dict(n=n, idx=idx, draws=np.array(list(zip(w0, w1)), dtype=np.uint64).reshape(len(idx), 1, 2), class_id=None)
    for n in (3, 1000):
        rng = np.random.default_rng(50 + n)
        B = 12
        idx = [0, n - 1] + rng.integers(0, n, B - 2).tolist()
        draws = rng.integers(0, 2 ** 32, (B, MAX_DRAWS, 2)).astype(np.uint64)
        one_other = np.zeros(n, dtype=np.int32)              # a single item of another class: most attempts are redrawn
        one_other[n // 2] = 1
        out[f"one_other_class_n{n}"] = dict(n=n, idx=idx, draws=draws, class_id=one_other)
        out[f"all_one_class_n{n}"] = dict(n=n, idx=idx, draws=draws, class_id=np.zeros(n, dtype=np.int32))     # exhausts the 300 draws
        out[f"many_classes_n{n}"] = dict(n=n, idx=idx, draws=draws, class_id=rng.integers(0, 3, n).astype(np.int32))
    return out


# ---------------------------------------------------------------------------------------------------- pair batches
# (N, S, F) of the pair-assembly test, each in every encoding, from an aligned bank and from a view of it that starts PAIR_VIEW_OFFSET
# elements in (off the 16-byte alignment).  N F = 20500 in f32: two chunks, the last one unrolled round and a 5-vector remainder; 36936
# in f16: a last chunk of 521 vectors, no whole round.  test_bank_cases_cpu.py shows which branches of the shared copy the list reaches.
PAIR_SHAPES = [(3, 5, 8), (16, 45, 2048), (5, 7, 9), (5, 7, 4100), (9, 7, 4104)]
PAIR_DTYPES = ("f32", "f16", "bf16")
PAIR_VIEW_OFFSET = 1


def assemble(txt_ids, txt_len, img_feats, img_pos, pairs):
    """the assembled batch of mv_pair_assemble"""
    pairs = np.asarray(pairs)
    im, tx = pairs[:, 0], pairs[:, 1]
    N = img_feats.shape[1]
    ln = np.asarray(txt_len)[tx].astype(np.int32)
    desc = np.stack([np.full(len(pairs), FAMILY_1D), np.full(len(pairs), N + 2), N + 2 + ln], axis=1).astype(np.int32)
    return dict(input_txt=np.asarray(txt_ids)[tx], segment=np.ones((len(pairs), txt_ids.shape[1]), dtype=np.int64), n_ids=ln, desc=desc,
                feats=np.asarray(img_feats)[im], pos=np.asarray(img_pos)[im])


def make_banks(n_txt, n_img, N, S, F, seed, vocab=1000):
    """text rows laid out as data_processing does (tokens + [SEP] = 102 + [PAD] = 0 ...), lengths from 1 to S+1 (both ends present)"""
    rng = np.random.default_rng(seed)
    T = S + 1
    lens = rng.integers(1, T + 1, n_txt).astype(np.int32)
    lens[0], lens[-1] = 1, T
    ids = np.zeros((n_txt, T), dtype=np.int64)
    for i, l in enumerate(lens.tolist()):
        ids[i, :l - 1] = rng.integers(200, vocab, l - 1)
        ids[i, l - 1] = 102
    feats = rng.standard_normal((n_img, N, F)).astype(np.float32)
    pos = np.sort(rng.integers(0, 49, (n_img, N)), axis=1).astype(np.int64)
    return ids, lens, feats, pos
