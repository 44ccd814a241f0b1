"""Shared definitions of the BLEU tests (no GPU, no package import): two references of what csrc/mv_bleu.hip computes and the named
cases of its sweeps.

The rule (include/medvill.h).  The reference evaluates report generation (Downstream_task/report_generation_and_vqa/sc/
generation_decode.py:480-498, detokenize :97-104, sc/bleu.py:16-64) by cutting the generated tokens at the first [SEP] / [PAD], merging
'##' pieces into the word before them -- a leading '##x' stays as it is --, joining with ' ', splitting on ' ' and handing the word
lists to nltk's corpus_bleu against gt_caption.split(' ').  corpus_bleu sums, per order o = 1..4, the clipped o-gram matches (numerator)
and max(1, Lh - o + 1) (denominator) over the samples, and the two lengths.

  string reference       `hyp_words` / `string_counts`: that rule on Python strings with collections.Counter; shares nothing with the
                         package (report_eval) and knows nothing of keys.
  key-level restatement  `word_keys` / `key_counts`: the two kernels' rules in NumPy on 64-bit keys, word by word.  `defect=` plants a
                         mistake the comparison with the string reference must catch (test_bleu_cases_cpu.py).

Cases are named after what they reach; `census` recomputes from a case's data what it reaches.  Shapes are tiny (V = 40, T <= 16,
n <= 8) but for the two long-row cases, one sample each."""
from collections import Counter

import numpy as np

MASK64 = (1 << 64) - 1
P = 0x9E3779B97F4A7C15          # the package's multiplier, restated (test_bleu_cases_cpu.py compares the two)
NT = 256                        # threads of a kernel block: the position loop of mv_bleu_counts takes a second pass past it
MAX_WORDS = 1024
NORD, NCOUNT = 4, 10
DEFECTS = ("strip_leading", "den_without_max", "no_clipping", "empty_is_zero_words")

TOKENS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "cat", "sat", "on", "mat", ".", ",", "no", "pleural", "eff", "##usion",
          "##s", "card", "##io", "##meg", "##aly", "disease", "heart", "size", "is", "normal", "##.", "##", "lung", "œd", "##ème", "肺",
          "##炎", "opacité", "a", "of", "effusion", "x", "##x", "##y"]
V = len(TOKENS)
PAD, SEP = TOKENS.index("[PAD]"), TOKENS.index("[SEP]")
ID = {t: i for i, t in enumerate(TOKENS)}


# ------------------------------------------------------------------------------------------------ the string reference
def hyp_words(row, tokens=TOKENS):
    """generation_decode.py:482-490 and bleu.py:43 for one row of ids: -> the list of words.  An id outside the vocabulary ends the row
    as [PAD] does (the decoder cannot produce one)."""
    kept = []
    for i in row:
        i = int(i)
        if i < 0 or i >= len(tokens) or tokens[i] in ("[SEP]", "[PAD]"):
            break
        kept.append(tokens[i])
    r_list = []
    for tk in kept:                                       # detokenize
        if tk.startswith("##") and len(r_list) > 0:
            r_list[-1] = r_list[-1] + tk[2:]
        else:
            r_list.append(tk)
    return " ".join(r_list).split(" ")


def _ngrams(words, o):
    return Counter(tuple(words[i:i + o]) for i in range(len(words) - o + 1))


def string_counts(hyps, refs):
    """corpus_bleu's sums over (hypothesis words, reference words) pairs: [num_1..4, den_1..4, hyp_len, ref_len] as Python ints
    (nltk's modified_precision with one reference: clipped counts over max(1, number of hypothesis o-grams))."""
    c = [0] * NCOUNT
    for h, r in zip(hyps, refs):
        for o in range(1, NORD + 1):
            ch, cr = _ngrams(h, o), _ngrams(r, o)
            c[o - 1] += sum(min(k, cr[g]) for g, k in ch.items())
            c[NORD + o - 1] += max(1, sum(ch.values()))
        c[8] += len(h)
        c[9] += len(r)
    return c


def case_string_counts(case, tokens=TOKENS):
    """The string reference over a case: row i against the reference text of item idx[i], clamped into the bank."""
    n_items = len(case["refs"])
    refs = [case["refs"][min(max(int(d), 0), n_items - 1)].split(" ") for d in case["idx"]]
    return string_counts([hyp_words(r, tokens) for r in case["ids"]], refs)


# ------------------------------------------------------------------------------------------------ keys
def key_of(s):
    k = 0
    for b in s.encode("utf-8"):
        k = (k * P + b) & MASK64
    return k


def tables(tokens=TOKENS):
    """tok_key, tail_key, tail_pow as lists of Python ints (unsigned), and empty_key."""
    cont = [t.startswith("##") for t in tokens]
    return dict(tok_key=[key_of(t) for t in tokens], tail_key=[key_of(t[2:]) if c else 0 for t, c in zip(tokens, cont)],
                tail_pow=[pow(P, len(t[2:].encode("utf-8")), 1 << 64) if c else 0 for t, c in zip(tokens, cont)], empty_key=key_of(""))


def as_i64(values):
    return np.array(values, dtype=np.uint64).view(np.int64)


def keyed_texts(texts):
    """text.split(' ') per text as key rows: (int64 [n, W] padded with 0, int32 [n])."""
    rows = [[key_of(w) for w in t.split(" ")] for t in texts]
    out = np.zeros((len(rows), max(len(r) for r in rows)), np.uint64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out.view(np.int64), np.array([len(r) for r in rows], np.int32)


# ------------------------------------------------------------------------------------------------ the key-level restatement
def word_keys(ids, tb, n_vocab, eos_id, pad_id, defect=None):
    """mv_bleu_words: ids int64 [n, T] -> (word_key int64 [n, T] with 0 behind the words, n_words int32 [n])."""
    ids = np.asarray(ids)
    n, T = ids.shape
    out, cnt = np.zeros((n, T), np.uint64), np.zeros(n, np.int32)
    for i in range(n):
        words = []
        for t in range(T):
            d = int(ids[i, t])
            if d == eos_id or d == pad_id or d < 0 or d >= n_vocab:
                break
            pw = tb["tail_pow"][d]
            if pw != 0 and t > 0:
                words[-1] = (words[-1] * pw + tb["tail_key"][d]) & MASK64
            elif pw != 0 and defect == "strip_leading":
                words.append(tb["tail_key"][d])
            else:
                words.append(tb["tok_key"][d])
        if not words and defect != "empty_is_zero_words":
            words = [tb["empty_key"]]
        out[i, :len(words)] = words
        cnt[i] = len(words)
    return out.view(np.int64), cnt


def _gram_eq(a, b, o):
    """bool [len(a) - o + 1, len(b) - o + 1]: the o keys from a[p] on equal those from b[q] on, one by one."""
    na, nb = max(len(a) - o + 1, 0), max(len(b) - o + 1, 0)
    m = np.ones((na, nb), bool)
    for k in range(o if na and nb else 0):
        m &= a[k:k + na, None] == b[None, k:k + nb]
    return m


def key_counts(hyp_key, hyp_n, ref_key, ref_n, idx, counters=None, defect=None):
    """mv_bleu_counts: per sample and order, every hypothesis position that is the first occurrence of its o-gram adds
    min(occurrences in the hypothesis, occurrences in the reference), the o keys compared one by one; -> uint64-valued Python ints
    [10], added to `counters` when given."""
    c = [0] * NCOUNT if counters is None else [int(v) for v in counters]
    n_items = len(ref_n)
    for i in range(len(hyp_n)):
        d = min(max(int(idx[i]), 0), n_items - 1)
        Lh, Lr = min(max(int(hyp_n[i]), 0), hyp_key.shape[1]), min(max(int(ref_n[d]), 0), ref_key.shape[1])
        h, r = hyp_key[i, :Lh], ref_key[d, :Lr]
        for o in range(1, NORD + 1):
            hh, hr = _gram_eq(h, h, o), _gram_eq(h, r, o)            # [position p, position q]: the o-grams at p and q are equal
            first = ~np.tril(hh, -1).any(axis=1)
            ch, cr = hh.sum(axis=1), hr.sum(axis=1)
            c[o - 1] += int((ch if defect == "no_clipping" else np.minimum(ch, cr))[first].sum())
            c[NORD + o - 1] += Lh - o + 1 if defect == "den_without_max" else max(1, Lh - o + 1)
        c[8] += Lh
        c[9] += Lr
    return c


def case_key_counts(case, defect=None, tokens=TOKENS):
    """The key-level restatement over a case, end to end: ids -> word keys -> counters against the keyed reference texts."""
    hk, hn = word_keys(case["ids"], tables(tokens), len(tokens), SEP, PAD, defect=defect)
    rk, rn = keyed_texts(case["refs"])
    return key_counts(hk, hn, rk, rn, case["idx"], defect=defect)


# ------------------------------------------------------------------------------------------------ cases
def row(text, T, end="[SEP]"):
    """'the cat ##s' -> ids of the tokens, then `end` (None: nothing), then [PAD] up to T."""
    ids = [ID[t] for t in text.split()] + ([ID[end]] if end else [])
    assert len(ids) <= T, (text, T)
    return ids + [PAD] * (T - len(ids))


def _case(name, rows, refs, idx=None):
    ids = np.array(rows, np.int64)
    idx = np.arange(len(rows), dtype=np.int32) if idx is None else np.array(idx, np.int32)
    return dict(name=name, ids=ids, refs=list(refs), idx=idx)


def _long(name, Lh, Lr, seed):
    """One sample of Lh one-token words against Lr reference words over the same few words: many repeats at every order."""
    g = np.random.default_rng(seed)
    words = ["the", "cat", "sat", "on", "mat", ".", "no", "is"]
    hyp = g.integers(0, len(words), Lh)
    ref = hyp[:Lr].copy() if Lr <= Lh else np.concatenate([hyp, g.integers(0, len(words), Lr - Lh)])
    flip = g.random(Lr) < 0.2
    ref[flip] = g.integers(0, len(words), int(flip.sum()))
    return _case(name, [[ID[words[k]] for k in hyp]], [" ".join(words[k] for k in ref)])


def cases():
    T = 8
    return [
        _case("empty_hypothesis", [[PAD] * T], ["the cat"]),
        _case("hypothesis_shorter_than_each_order", [row("the", T), row("the cat", T), row("the cat sat", T)], ["the cat sat on the mat ."] * 3),
        _case("reference_shorter_than_each_order", [row("the cat sat on the mat", T)] * 3, ["the", "the cat", "the cat sat"]),
        _case("row_without_sep_full_T", [row("the cat sat on the mat . no", T, end=None)], ["the cat sat on the mat . no"]),
        _case("sep_at_column_0", [[SEP] + row("the cat", T - 1)], ["the cat"]),
        _case("pad_before_sep", [[ID["the"], ID["cat"], PAD, ID["sat"], SEP, PAD, PAD, PAD]], ["the cat sat"]),
        _case("leading_continuation", [row("##usion the", T), row("##usion the", T)], ["##usion the", "usion the"]),
        _case("lone_continuation", [row("the ## cat", T), row("## cat", T)], ["the cat", "## cat"]),
        _case("continuations_to_the_end_of_the_row", [row("eff ##usion ##s ##s ##s ##s ##s ##s", T, end=None)], ["effusionssssss"]),
        _case("assembled_word_equals_single_token_and_raw_word", [row("no eff ##usion", T), row("card ##io ##meg ##aly", T)],
              ["no effusion", "cardiomegaly"]),
        _case("reference_punctuation_does_not_match", [row("heart disease .", T), row("heart disease ##.", T)], ["heart disease."] * 2),
        _case("unk_against_a_raw_word", [row("[UNK] is normal", T), row("[UNK] is normal", T)], ["Heart is normal", "[UNK] is normal"]),
        _case("double_spaces_in_the_reference", [row("the cat", T), [PAD] * T], ["the  cat ", " the cat"]),
        _case("clipping", [row("the the the the", T)], ["the cat the"]),
        _case("repeated_higher_order_ngram", [row("the cat the cat the cat", T)], ["the cat the cat"]),
        _long("hypothesis_longer_than_a_block", NT + 44, NT + 24, seed=1),
        _long("both_rows_at_the_cap", MAX_WORDS, MAX_WORDS, seed=2),
        _case("id_outside_the_vocabulary", [[ID["the"], ID["cat"], V + 3, ID["sat"], SEP, PAD, PAD, PAD],
                                            [ID["the"], -1, ID["cat"], SEP, PAD, PAD, PAD, PAD]], ["the cat sat", "the cat"]),
        _case("idx_repeats_and_leaves_the_bank", [row("the cat", T), row("the mat", T), row("no cat", T), row("the cat sat", T),
                                                  row("on the mat", T), row("cat", T)], ["the cat sat", "on the mat", "no cat"],
              idx=[0, 0, 2, -5, 7, 1]),
        _case("non_ascii_tokens", [row("œd ##ème 肺 ##炎 opacité", T)], ["œdème 肺炎 opacité"]),
    ]


def census(case, tokens=TOKENS):
    """What a case reaches, recomputed from its data: a set of tags."""
    tags = set()
    ids, refs, idx = case["ids"], case["refs"], case["idx"]
    n_items, T = len(refs), ids.shape[1]
    vocab = set(tokens)
    if len(set(idx.tolist())) < len(idx) and (idx.min() < 0 or idx.max() >= n_items):
        tags.add("idx_clamp")
    for i, r in enumerate(ids):
        ref = refs[min(max(int(idx[i]), 0), n_items - 1)].split(" ")
        hyp = hyp_words(r, tokens)
        stop = [t for t, d in enumerate(r) if d < 0 or d >= len(tokens) or tokens[d] in ("[SEP]", "[PAD]")]
        end = stop[0] if stop else T
        kept = [tokens[d] for d in r[:end]]
        tags.add(f"hyp_len_{len(hyp)}" if len(hyp) < NORD else "hyp_len_4+")
        tags.add(f"ref_len_{len(ref)}" if len(ref) < NORD else "ref_len_4+")
        if hyp == [""]:
            tags.add("empty_hyp")
        if end == T:
            tags.add("full_T")
            if kept[-1].startswith("##") and len(kept) > 1:
                tags.add("cont_to_end")
        if r[0] == SEP:
            tags.add("sep_col0")
        if stop and r[stop[0]] == PAD and SEP in r[stop[0]:].tolist():
            tags.add("pad_before_sep")
        if stop and not 0 <= r[stop[0]] < len(tokens):
            tags.add("id_oob")
        if kept and kept[0].startswith("##"):
            tags.add("leading_cont")
        if "##" in kept:
            tags.add("lone_cont")
        if "[UNK]" in hyp:
            tags.add("unk")
        if any(ord(ch) > 127 for t in kept for ch in t):
            tags.add("non_ascii")
        assembled = set(hyp) - vocab
        if any(w in vocab for w in ref if w in set(hyp) and w not in kept):
            tags.add("assembled_single")
        if assembled & set(ref):
            tags.add("assembled_raw")
        if any(w + "." in ref and w not in ref for w in hyp):
            tags.add("punct_mismatch")
        if "" in ref and len(ref) > 1:
            tags.add("empty_ref_word")
        h1, r1 = _ngrams(hyp, 1), _ngrams(ref, 1)
        if any(0 < r1[g] < k for g, k in h1.items()):
            tags.add("clipped")
        if any(k >= 2 for o in (2, 3, 4) for k in _ngrams(hyp, o).values()):
            tags.add("repeat_high")
        if len(hyp) > NT:
            tags.add("multi_pass")
        if len(hyp) == len(ref) == MAX_WORDS:
            tags.add("at_cap")
    return tags


# the tags each named case must reach (test_bleu_cases_cpu.py)
REACHES = {
    "empty_hypothesis": {"empty_hyp"},
    "hypothesis_shorter_than_each_order": {"hyp_len_1", "hyp_len_2", "hyp_len_3"},
    "reference_shorter_than_each_order": {"ref_len_1", "ref_len_2", "ref_len_3"},
    "row_without_sep_full_T": {"full_T"},
    "sep_at_column_0": {"sep_col0", "empty_hyp"},
    "pad_before_sep": {"pad_before_sep"},
    "leading_continuation": {"leading_cont"},
    "lone_continuation": {"lone_cont", "leading_cont"},
    "continuations_to_the_end_of_the_row": {"cont_to_end", "full_T"},
    "assembled_word_equals_single_token_and_raw_word": {"assembled_single", "assembled_raw"},
    "reference_punctuation_does_not_match": {"punct_mismatch"},
    "unk_against_a_raw_word": {"unk"},
    "double_spaces_in_the_reference": {"empty_ref_word", "empty_hyp"},
    "clipping": {"clipped"},
    "repeated_higher_order_ngram": {"repeat_high"},
    "hypothesis_longer_than_a_block": {"multi_pass", "repeat_high", "clipped"},
    "both_rows_at_the_cap": {"at_cap", "multi_pass"},
    "id_outside_the_vocabulary": {"id_oob"},
    "idx_repeats_and_leaves_the_bank": {"idx_clamp"},
    "non_ascii_tokens": {"non_ascii", "assembled_raw"},
}
