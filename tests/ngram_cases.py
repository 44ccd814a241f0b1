"""Cases, restated dispatch, references and bounds of the n-gram blocking kernels (csrc/mv_decode.hip: mv_ngram_ban,
mv_logprob_topk_banned), in the shape of tests/decode_cases.py, from which the top-k value grid, vocabularies and bounds come.

Plain module: nothing here touches the GPU or the HIP library.  tests/test_ngram_sweep_gpu.py runs the cases,
tests/test_ngram_cases_cpu.py counts the branches they reach, checks the constants against the source and plants defects.

* `banned_words` is the rule in plain Python, written from its description; `blocked_beam` drives
  medvill_amd.beam.BeamSearch with it, the way generate() drives the two kernels;
* every generator draws from np.random.RandomState(fixed + seed) and returns a dict that reproduces the case;
* the branch names of a case are observed on the sequences / logits the case really holds, not on what the generator meant to plant.
"""
import numpy as np
import torch

import decode_cases as D

# ---- constants of csrc/mv_decode.hip (tests/test_ngram_cases_cpu.py reads the same numbers out of the source and the header) ----
NB_MAX_LEN = 1024             # words of one history, the new one included
NB_MAX_IGN = 256
NB_MIN_N, NB_MAX_N = 2, 8
NB_THREADS = 256
TKB_MAX_V = 131072
BAN_PENALTY = -10000.0
PENALTY_HALF_ULP = 2.0 ** -11  # half an f32 ulp in [8192, 16384): the one extra rounding of fl(logp - 10000)

HIST_SENTINEL = -7777777
BAN_SENTINEL = -8888888
NBAN_SENTINEL = -9999999
GUARD_ROWS = 2


# =====================================================================================================================
# the rule
# =====================================================================================================================
def banned_words(seq, n, ignore=None, defect=None):
    """Words that may not follow `seq` (a list of ids): those that would complete an n-gram `seq` already holds.  Ascending, each once.
    defect (tests only): 'no_dedup', 'no_ignore_tail', 'short_last_window' plant the bugs test_ngram_cases_cpu.py must see."""
    ignore = set(ignore or ())
    L = len(seq)
    if L < n:
        return []
    tail = seq[L - (n - 1):]
    if defect != "no_ignore_tail" and any(w in ignore for w in tail):
        return []
    out = []
    last = L - n - (1 if defect == "short_last_window" else 0)
    for i in range(last + 1):
        if seq[i:i + n - 1] == tail and seq[i + n - 1] not in ignore:
            out.append(seq[i + n - 1])
    return sorted(out) if defect == "no_dedup" else sorted(set(out))


def step_histories(seqs, parents, words):
    """seqs: list of lists per beam; -> the new lists: the parent's words plus the chosen word"""
    return [list(seqs[int(p)]) + [int(w)] for p, w in zip(parents, words)]


def blocked_beam(tables, B, K, eos_id, min_len, length_penalty, max_len, n, ignore=None, record=None):
    """Beam search with n-gram blocking through medvill_amd.beam.BeamSearch: tables[t] = log_softmax of step t's scores, f32
    [B*K, V] (at step 0 row b*K is sample b's only beam).  n = 0: no blocking.  -> BeamSearch.finalize(max_len)."""
    from medvill_amd.beam import BeamSearch
    bs = BeamSearch(B, K, eos_id, length_penalty)
    seqs = [[] for _ in range(B * K)]
    for t, lt in enumerate(tables):
        lp = lt.clone().float()
        for r, s in enumerate(seqs):
            for w in (banned_words(s, n, ignore) if n else []):
                lp[r, w] += BAN_PENALTY
        if t < min_len:
            lp[:, eos_id] = BAN_PENALTY
        vals, idx = torch.topk(lp, k=K)
        back, k_ids = bs.step(vals, idx)
        if t == 0:
            seqs = [[int(w)] for w in k_ids.reshape(-1)]
        else:
            seqs = step_histories(seqs, bs.parents(back), k_ids.reshape(-1))
        if record is not None:
            record.append([list(s) for s in seqs])
    return bs.finalize(max_len)


def has_repeated_ngram(seq, n):
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) != len(set(grams))


# =====================================================================================================================
# mv_ngram_ban
# =====================================================================================================================
NB_L = (63, 64, 65, 255, 256, 257, 511, 512, NB_MAX_LEN)                  # len + 1 around the block's strides, and the cap
NB_KINDS = ("random", "unique", "one_match", "dedup", "run", "last_window_only", "ignore_in_tail", "ignore_candidate", "two_words")
NB_PARENT = ("parent_null", "parent_perm", "parent_shared")
NB_R = (1, 3, 4, 12)
N_NB = 108


def nb_case(seed):
    rs = np.random.RandomState(9100 + seed)
    n = NB_MIN_N + seed % (NB_MAX_N - NB_MIN_N + 1)
    third = seed % 3
    if third == 0:
        L = int(NB_L[(seed // 3) % len(NB_L)])
    elif third == 1:
        L = max(1, n + (-1, 0, 1)[(seed // 3) % 3])                           # just below, at and above n
    else:
        L = int(rs.randint(n + 1, 40))
    wide = bool((seed // 2) % 2)
    need = max(L + 1 - n, 0)
    return dict(fam="nb", seed=seed, n=n, L=L, R=int(NB_R[(seed + seed // 4) % len(NB_R)]), parent=NB_PARENT[(seed + seed // 3) % 3],
                ld_h=L + (int(rs.choice([1, 5, 64])) if wide else 0), ld_ban=need + (int(rs.choice([1, 3, 17])) if wide or need == 0 else 0),
                n_ign=int((0, 1, 3, NB_MAX_IGN)[(seed // 5) % 4]))


def nb_cases():
    return [nb_case(s) for s in range(N_NB)]


def _nb_sequence(rs, kind, L, n, ign):
    """one new history of L words that shows `kind` where L leaves room for it (a random one otherwise).  Words that are not planted
    are distinct and above 1000; the ignore ids `ign` are in 500..999."""
    base = (1000 + rs.permutation(4 * L + 16)[:L]).tolist()
    if kind == "random" or L < n + 1:
        small = int(rs.randint(2, 5))
        return rs.randint(1, 1 + small, size=L).tolist()
    tail = base[L - (n - 1):]
    room = L - (n - 1) - n              # first index a planted copy of the tail may not pass (copy + its follower end before the tail)
    if kind == "unique":
        return base
    if kind in ("one_match", "ignore_candidate") and room >= 0:
        i = int(rs.randint(room + 1))
        base[i:i + n - 1] = tail
        if kind == "ignore_candidate" and len(ign):
            base[i + n - 1] = int(ign[0])
        return base
    if kind == "dedup" and room - n >= 0:
        base[0:n - 1] = tail
        base[n:2 * n - 1] = tail
        base[2 * n - 1] = base[n - 1]
        return base
    if kind == "two_words" and room - n >= 0:
        base[0:n - 1] = tail
        base[n:2 * n - 1] = tail
        if base[2 * n - 1] > base[n - 1]:                                   # found in descending order: the list must come out ascending
            base[2 * n - 1], base[n - 1] = base[n - 1], base[2 * n - 1]
        return base
    if kind == "run":
        m = int(rs.randint(n, L + 1))
        return base[:L - m] + [7] * m
    if kind == "last_window_only":
        return base[:L - n] + [9] * n
    if kind == "ignore_in_tail" and len(ign):
        if rs.randint(2) and room >= 0:                                    # the tail holds an ignore word and stands earlier too:
            base[L - 1] = int(ign[-1])                                     # without the check its follower there would be banned
            base[0:n - 1] = base[L - (n - 1):]
            return base
        small = rs.randint(1, 3, size=L).tolist()
        small[L - 1 - int(rs.randint(n - 1))] = int(ign[-1])
        return small
    return base


def nb_inputs(cfg):
    """CPU tensors of a case: hist_in int32 [R, ld_h] (sentinels behind column len), parent int64 [R] or None, y int64 [R],
    ignore int32 [n_ign] or None, and the new histories `seqs` (lists) the kernel must produce."""
    rs = np.random.RandomState(9200 + cfg["seed"])
    R, L, n, ld_h = cfg["R"], cfg["L"], cfg["n"], cfg["ld_h"]
    ln = L - 1
    ign = (500 + rs.permutation(500)[:cfg["n_ign"]]).astype(np.int32)
    if cfg["parent"] == "parent_null":
        par = np.arange(R)
    elif cfg["parent"] == "parent_perm":
        par = rs.permutation(R)
    else:
        par = np.full(R, int(rs.randint(R)))
        if R > 2:
            par[R - 1] = (par[0] + 1) % R
    src = {}
    for p in sorted(set(par.tolist())):
        src[p] = _nb_sequence(rs, NB_KINDS[(cfg["seed"] + p) % len(NB_KINDS)], L, n, ign)
    hist = np.full((R, ld_h), HIST_SENTINEL, dtype=np.int32)
    for p in range(R):                                   # rows nobody descends from hold words too (they must not leak)
        hist[p, :ln] = src[p][:ln] if p in src else rs.randint(1, 4, size=ln)
    y = np.zeros(R, dtype=np.int64)
    seen = set()
    for r in range(R):
        p = int(par[r])
        y[r] = src[p][ln] if p not in seen else int(rs.choice([src[p][ln], 1 + int(rs.randint(4))]))
        seen.add(p)
    seqs = [hist[int(par[r]), :ln].tolist() + [int(y[r])] for r in range(R)]
    return dict(hist_in=torch.from_numpy(hist), parent=None if cfg["parent"] == "parent_null" else torch.from_numpy(par.astype(np.int64)),
                y=torch.from_numpy(y), ignore=torch.from_numpy(ign) if cfg["n_ign"] else None, seqs=seqs)


def nb_expected(cfg, inp, defect=None):
    """-> (ban lists per row, by the rule)"""
    ign = inp["ignore"].tolist() if inp["ignore"] is not None else None
    return [banned_words(s, cfg["n"], ign, defect) for s in inp["seqs"]]


def nb_branches(cfg):
    inp = nb_inputs(cfg)
    n, L = cfg["n"], cfg["L"]
    ign = set(inp["ignore"].tolist()) if inp["ignore"] is not None else set()
    b = ["n=%d" % n, cfg["parent"], "L<n" if L < n else ("L==n" if L == n else "L>n")]
    if L == n + 1:
        b.append("L==n+1")
    if L == n - 1:
        b.append("L==n-1")
    if L in NB_L:
        b.append("L=%d" % L)
    if cfg["ld_h"] > L:
        b.append("ld_h>L")
    if cfg["ld_ban"] > max(L + 1 - n, 0):
        b.append("ld_ban>need")
    b.append("ignore_none" if not ign else ("ignore_cap" if len(ign) == NB_MAX_IGN else "ignore_some"))
    if cfg["parent"] == "parent_shared" and cfg["R"] > 1:
        b.append("many_rows_one_parent")
    seen = set()
    for s in inp["seqs"]:
        if L < n:
            continue
        tail = s[L - (n - 1):]
        if any(w in ign for w in tail):
            seen.add("ignore_in_tail")
            if banned_words(s, n, ign, defect="no_ignore_tail"):
                seen.add("ignore_in_tail_hides_a_ban")
            continue
        hits = [i for i in range(L - n + 1) if s[i:i + n - 1] == tail]
        words = [s[i + n - 1] for i in hits]
        kept = [w for w in words if w not in ign]
        if len(kept) < len(words):
            seen.add("ignore_candidate")
        seen.add({0: "no_match", 1: "one_match"}.get(len(hits), "several_matches"))
        if len(kept) > len(set(kept)):
            seen.add("dedup")
        if len(set(kept)) >= 2:
            seen.add("several_words")
            if kept != sorted(kept):
                seen.add("found_out_of_order")
        if any(i + n - 1 >= L - (n - 1) for i in hits):                      # the repeated n-gram reaches into the tail: a run of one word
            seen.add("window_overlaps_tail")
        if hits == [L - n]:
            seen.add("last_window_only")
        if len(hits) > NB_THREADS:
            seen.add("more_windows_than_threads")
    return b + sorted(seen)


# =====================================================================================================================
# mv_logprob_topk_banned
# =====================================================================================================================
TKB_MODES = ("ban_null", "ban_empty", "ban_single", "ban_many", "ban_best", "ban_eos", "ban_out_of_range", "ban_collide", "ban_listed_twice")
TKB_COLLIDE_DELTA = 2.0 ** -13        # two banned logits this far apart: their penalised values round to one f32
TKB_BOUNDARY_CLEARANCE = 1e-4         # ... and neither lies this close to a rounding boundary of the penalised value
N_TKB = 108


def tkb_case(seed):
    c = dict(D.tk_case(seed % D.N_TK), fam="tkb", seed=seed, ban_mode=TKB_MODES[(seed + seed // 9) % len(TKB_MODES)])
    c["ld_ban"] = (1, 7, 64)[seed % 3] if c["ban_mode"] in ("ban_empty", "ban_single") else 64
    if c["ban_mode"] == "ban_collide":                   # banned columns are emitted only when k == V: the collision must be seen
        v = int((3, 5, 8, 16)[(seed // 9) % 4])
        c.update(V=v, k=v, ld=v + (0, 1, 8)[seed % 3])
    return c


TKB_FIXED = [dict(c, fam="tkb", ban_mode=m, ld_ban=64) for c, m in zip(D.TK_FIXED, ("ban_best", "ban_many", "ban_eos", "ban_single", "ban_collide", "ban_many"))]


def tkb_cases():
    return [tkb_case(s) for s in range(N_TKB)] + TKB_FIXED


def _pen32(lp64):
    """fl(fl(logp) - 10000) in f32 arithmetic, from an fp64 log-prob"""
    return (np.asarray(lp64, dtype=np.float64).astype(np.float32) + np.float32(BAN_PENALTY)).astype(np.float32).astype(np.float64)


def tkb_inputs(cfg):
    """-> (logits f32 [rows, ld] as decode_cases.tk_inputs makes them (two columns moved for ban_collide), ban int32 [rows, ld_ban] or
    None, nban int32 [rows] or None).  Columns of ban behind nban hold column 0..: a kernel that read them would ban real words."""
    x = D.tk_inputs(cfg)
    V, mode, ld_ban = cfg["V"], cfg["ban_mode"], cfg["ld_ban"]
    rows = x.shape[0]
    rs = np.random.RandomState(9300 + cfg["seed"])
    eos = D.tk_eos(cfg)
    if mode == "ban_null":
        return x, None, None
    ban = np.tile(np.arange(ld_ban, dtype=np.int32) % V, (rows, 1))
    nban = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        row = x[r, :V].double().numpy()
        lst = []
        if mode == "ban_single":
            lst = [int(rs.randint(V))]
        elif mode == "ban_many":
            lst = rs.permutation(V)[:min(V, int(rs.randint(2, 41)))].tolist()
        elif mode == "ban_best":
            lst = [int(np.argmax(row))] + rs.permutation(V)[:min(V, 3)].tolist()
        elif mode == "ban_eos":
            lst = [eos if 0 <= eos < V else int(np.argmax(row))] + rs.permutation(V)[:min(V, 2)].tolist()
        elif mode == "ban_out_of_range":
            lst = [-1, V, int(rs.randint(V)), V + 5, 2 ** 30, -2 ** 31]
        elif mode == "ban_listed_twice":
            c = int(rs.randint(V))
            lst = [c, int(rs.randint(V)), c]
        elif mode == "ban_collide" and V >= 3:
            fin = [c for c in rs.permutation(V).tolist() if np.isfinite(row[c]) and c != eos]
            for a in range(len(fin) - 1):
                c1, c2 = sorted(fin[a:a + 2])
                trial = row.copy()
                trial[c2] = trial[c1] + TKB_COLLIDE_DELTA                  # the higher column holds the (slightly) larger logit
                t32 = trial.astype(np.float32).astype(np.float64)
                lse = np.log(np.exp(t32[np.isfinite(t32)] - t32[np.isfinite(t32)].max()).sum()) + t32[np.isfinite(t32)].max()
                lo, hi = t32[c1] - lse, t32[c2] - lse
                if _pen32(lo - TKB_BOUNDARY_CLEARANCE) == _pen32(hi + TKB_BOUNDARY_CLEARANCE):
                    x[r, c2] = float(trial[c2])
                    lst = [c2, c1]
                    break
        lst = list(dict.fromkeys(lst)) if mode not in ("ban_listed_twice",) else lst
        lst = lst[:ld_ban]
        ban[r, :len(lst)] = lst
        nban[r] = len(lst)
    return x, torch.from_numpy(ban), torch.from_numpy(nban)


def tkb_reference(x64, k, eos, ban, nban, defect=None):
    """x64 fp64 [R, V] -> dict(vals fp64 [R, k] (banned: logp - 10000 unrounded), idx int64 [R, k], lse fp64 [R], banned bool [R, k],
    rank fp64 [R, min(V, k+1)] the values the order was made on (banned: fl(fl(logp) - 10000)), the k+1-th place included,
    lp fp64 [R, V] every column's value, mask bool [R, V] the banned columns (the penalised EOS column is not one)).
    defect (tests only): 'before_normalisation', 'fill'."""
    R, V = x64.shape
    mask = torch.zeros((R, V), dtype=torch.bool)
    if ban is not None:
        for r in range(R):
            for c in ban[r, :int(nban[r])].tolist():
                if 0 <= c < V:
                    mask[r, c] = True
    mask = mask.to(x64.device)
    if defect == "before_normalisation":
        xx = torch.where(mask, x64 + BAN_PENALTY, x64)
        lse = torch.logsumexp(xx, dim=-1)
        lp = xx - lse[:, None]
        rank = lp.clone()
    else:
        lse = torch.logsumexp(x64, dim=-1)
        lp = x64 - lse[:, None]
        pen = torch.full_like(lp, BAN_PENALTY) if defect == "fill" else lp + BAN_PENALTY
        rank = torch.where(mask, torch.from_numpy(_pen32(lp.cpu().numpy())).to(lp.device) if defect is None else pen, lp)
        lp = torch.where(mask, pen, lp)
    if 0 <= eos < V:
        lp[:, eos] = BAN_PENALTY
        rank[:, eos] = BAN_PENALTY
        mask[:, eos] = False
    order = torch.sort(-rank, dim=-1, stable=True).indices
    sel = order[:, :k]
    return dict(vals=lp.gather(1, sel), idx=sel, lse=lse, banned=mask.gather(1, sel), rank=rank.gather(1, order[:, :min(V, k + 1)]), lp=lp,
                mask=mask)


def tkb_bound(ref, tol, idx=None):
    """per entry of idx ([R, k]; default: the reference's selection): `tol` (decode_cases.case_tol, as for mv_logprob_topk) on the
    log-prob; a banned entry adds the rounding of fl(logp - 10000), half an ulp at that magnitude.  (The penalised EOS column and
    -inf log-probs are compared exactly by the caller.)"""
    banned = ref["mask"].gather(1, ref["idx"] if idx is None else idx)
    return torch.full(banned.shape, float(tol), dtype=torch.float64, device=banned.device) + banned.double() * PENALTY_HALF_ULP


def tkb_excused(ref, bound):
    """bool [R, k]: entries whose place in the order the reference cannot vouch for -- a neighbour (the k+1-th included) lies closer
    than the two bounds together without being an exact tie (exact ties go to the lower column and are asserted)."""
    rank = ref["rank"]
    R, k = ref["idx"].shape
    m = rank.shape[1]
    b = torch.cat([bound, bound[:, -1:] + PENALTY_HALF_ULP], dim=1)[:, :m]
    gap = (rank[:, :-1] - rank[:, 1:]).abs()
    gap = torch.where(torch.isnan(gap), torch.zeros_like(gap), gap)            # -inf next to -inf: a tie
    close = (gap > 0) & (gap <= b[:, :-1] + b[:, 1:])
    ex = torch.zeros((R, k), dtype=torch.bool, device=rank.device)
    for j in range(m - 1):
        if j < k:
            ex[:, j] |= close[:, j]
        if j + 1 < k:
            ex[:, j + 1] |= close[:, j]
    return ex


def tkb_branches(cfg):
    x, ban, nban = tkb_inputs(cfg)
    V, k = cfg["V"], cfg["k"]
    eos = D.tk_eos(cfg)
    x64 = x[:, :V].double()
    ref = tkb_reference(x64, k, eos, ban, nban)
    plain = D.tk_reference(x64, k, eos)
    b = ["km%d" % D.tk_km(k), cfg["ban_mode"]]
    if k == V:
        b.append("k==V")
    if bool(ref["banned"].any()):
        b.append("banned_column_emitted")
    if not torch.equal(ref["idx"], plain[1]):
        b.append("selection_changed_by_ban")
    if ban is not None:
        lists = [ban[r, :int(nban[r])].tolist() for r in range(ban.shape[0])]
        if any(c < 0 or c >= V for l in lists for c in l):
            b.append("id_out_of_range")
        if any(len(l) != len(set(l)) for l in lists):
            b.append("id_listed_twice")
        if 0 <= eos < V and any(eos in l for l in lists):
            b.append("eos_banned_and_penalised")
        if any(int(torch.argmax(x64[r])) in l for r, l in enumerate(lists)):
            b.append("best_column_banned")
        if any(len(l) > 16 for l in lists):
            b.append("more_bans_than_a_list_holds")
        if cfg["ld_ban"] > int(nban.max()):
            b.append("ld_ban>nban")
    rk, sel = ref["rank"], ref["idx"]
    for r in range(sel.shape[0]):
        for o in range(min(k, rk.shape[1]) - 1):
            if bool(ref["banned"][r, o]) and bool(ref["banned"][r, o + 1]) and float(rk[r, o]) == float(rk[r, o + 1]) \
                    and float(x64[r, sel[r, o]]) != float(x64[r, sel[r, o + 1]]):
                b.append("penalised_values_collide")
    return sorted(set(b))


FAMILIES = {"nb": (nb_cases, nb_branches), "tkb": (tkb_cases, tkb_branches)}


def census(fam):
    cases, branches = FAMILIES[fam]
    count = {}
    for c in cases():
        for name in branches(c):
            count[name] = count.get(name, 0) + 1
    return count
