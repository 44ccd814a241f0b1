"""The BLEU evaluation's host side and the case set of its sweeps, without a GPU: the word tables obey the concatenation law, the
key-level restatement of the two kernels (tests/bleu_cases.py) equals the string reference on every named case as exact integers, every
case reaches the branch it is named after, each planted defect is caught by some case, and report_eval.bleu_from_counters is nltk's
corpus_bleu formula (literal transcription, hand-computed corpora, and nltk itself where it is installed)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd  # noqa: F401,E402
from medvill_amd import report_eval as RE     # noqa: E402
import bleu_cases as C                        # noqa: E402

CASES = C.cases()
SMALL = [c for c in CASES if c["ids"].shape[1] <= 16]
FMIN = sys.float_info.min


def _u64(t):
    return [int(v) & C.MASK64 for v in torch.as_tensor(t).reshape(-1).tolist()]


def test_the_tables_obey_the_concatenation_law_over_random_splits():
    assert RE.P == C.P and RE.P % 2 == 1
    g = np.random.default_rng(0)
    alphabet = list("abcxyz.,-é肺œ ") + ["##"]
    for _ in range(200):
        s = "".join(g.choice(alphabet, int(g.integers(0, 12))))
        cut = int(g.integers(0, len(s) + 1))
        a, b = s[:cut], s[cut:]
        want = (RE.str_key(a) * pow(RE.P, len(b.encode("utf-8")), 1 << 64) + RE.str_key(b)) & C.MASK64
        assert RE.str_key(s) == want == C.key_of(s), (a, b)
    # the same law through the tables: a word assembled from a start token and continuation tokens
    tb = RE.word_tables(C.TOKENS)
    ref = C.tables()
    for k in ("tok_key", "tail_key", "tail_pow"):
        assert tb[k].dtype == torch.int64 and _u64(tb[k]) == ref[k], k
    assert tb["empty_key"] == ref["empty_key"] == RE.str_key("") == 0
    tok, tail, pw = (_u64(tb[k]) for k in ("tok_key", "tail_key", "tail_pow"))
    starts = [i for i, t in enumerate(C.TOKENS) if not t.startswith("##")]
    conts = [i for i, t in enumerate(C.TOKENS) if t.startswith("##")]
    assert all(pw[i] == 0 for i in starts) and all(pw[i] != 0 for i in conts)      # the lone '##': P^0 = 1, still a continuation
    for _ in range(100):
        ids = [int(g.choice(starts))] + [int(v) for v in g.choice(conts, int(g.integers(0, 5)))]
        key = tok[ids[0]]
        for i in ids[1:]:
            key = (key * pw[i] + tail[i]) & C.MASK64
        assert key == RE.str_key(C.TOKENS[ids[0]] + "".join(C.TOKENS[i][2:] for i in ids[1:]))


def test_word_tables_refuse_tokens_that_would_change_the_word_count():
    for bad in (["a", ""], ["a b"], [" "], []):
        with pytest.raises(ValueError):
            RE.word_tables(bad)


def test_text_keys_split_exactly():
    keys, counts = RE.text_keys(["the  cat ", "", "The", " x"])
    assert counts.tolist() == [4, 1, 1, 2] and tuple(keys.shape) == (4, 4)
    k = RE.str_key
    assert _u64(keys[0]) == [k("the"), 0, k("cat"), 0] and _u64(keys[1])[0] == 0
    assert _u64(keys[2])[0] == k("The") != k("the")                                # nothing is lower-cased
    want, n = C.keyed_texts(["the  cat ", "", "The", " x"])
    assert np.array_equal(keys.numpy(), want) and counts.tolist() == n.tolist()


def test_decode_text_is_the_reference_join():
    for c in SMALL:
        inside = np.where((c["ids"] < 0) | (c["ids"] >= C.V), C.PAD, c["ids"])       # (decode_text indexes the vocabulary: ids inside it)
        assert RE.decode_text(torch.from_numpy(inside), C.TOKENS) == [" ".join(C.hyp_words(r)) for r in c["ids"]], c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_key_level_restatement_equals_the_string_reference(case):
    want = C.case_string_counts(case)
    assert C.case_key_counts(case) == want
    hk, hn = C.word_keys(case["ids"], C.tables(), C.V, C.SEP, C.PAD)
    for i, r in enumerate(case["ids"]):                                            # word by word: the keys of the reference's strings
        words = C.hyp_words(r)
        assert hn[i] == len(words)
        assert [int(v) & C.MASK64 for v in hk[i, :hn[i]]] == [C.key_of(w) for w in words] and not hk[i, hn[i]:].any()


def test_every_named_case_reaches_its_branch_and_shapes_stay_tiny():
    assert {c["name"] for c in CASES} == set(C.REACHES) and len(CASES) == 20
    for c in CASES:
        assert C.REACHES[c["name"]] <= C.census(c), (c["name"], C.census(c))
        n, T = c["ids"].shape
        assert (n <= 8 and T <= 16) or (n == 1 and T <= C.MAX_WORDS), c["name"]
    assert C.V <= 64 and len(CASES) - len(SMALL) == 2
    # hand-checked figures of three cases
    by = {c["name"]: C.case_string_counts(c) for c in CASES}
    assert by["clipping"] == [2, 0, 0, 0, 4, 3, 2, 1, 4, 3]
    assert by["empty_hypothesis"] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 2]
    assert by["double_spaces_in_the_reference"][:2] == [3, 0]                      # 'the', 'cat', the empty hypothesis' ''; 'the cat' is not adjacent


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_a_planted_defect_is_caught_by_some_case(defect):
    caught = [c["name"] for c in SMALL if C.case_key_counts(c, defect=defect) != C.case_string_counts(c)]
    assert caught, defect


# ------------------------------------------------------------------------------------------------ bleu_from_counters
def _transcription(c):
    """The formula of the issue, line by line."""
    num, den, hyp_len, ref_len = c[0:4], c[4:8], c[8], c[9]
    out = {}
    for name, w in (("bleu1", (1, 0, 0, 0)), ("bleu2", (.5, .5, 0, 0)), ("bleu3", (.33, .33, .33, 0)), ("bleu4", (.25, .25, .25, .25))):
        if hyp_len > ref_len:
            bp = 1.0
        elif hyp_len == 0:
            bp = 0.0
        else:
            bp = math.exp(1 - ref_len / hyp_len)
        if num[0] == 0:
            out[name] = 0.0
            continue
        p = [num[o] / den[o] if num[o] != 0 else FMIN for o in range(4)]
        out[name] = bp * math.exp(math.fsum(w[o] * math.log(p[o]) for o in range(4)))
    return out


def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * abs(b)


def test_bleu_from_counters_equals_the_transcription():
    g = np.random.default_rng(3)
    sets = [C.case_string_counts(c) for c in CASES]
    for _ in range(50):
        den = sorted((int(v) for v in g.integers(1, 1000, 4)), reverse=True)
        sets.append([int(g.integers(0, d + 1)) for d in den] + den + [int(g.integers(0, 1200)), int(g.integers(1, 1200))])
    for c in sets:
        got, want = RE.bleu_from_counters(torch.tensor(c, dtype=torch.int64)), _transcription(c)
        assert set(got) == {"bleu1", "bleu2", "bleu3", "bleu4"}
        for k in want:
            assert isinstance(got[k], float) and _close(got[k], want[k]), (c, k, got[k], want[k])


def test_bleu_from_counters_on_three_hand_computed_corpora():
    f = RE.bleu_from_counters
    # no unigram matches: every score is 0
    assert f([0, 0, 0, 0, 3, 2, 1, 1, 3, 3]) == dict(bleu1=0.0, bleu2=0.0, bleu3=0.0, bleu4=0.0)
    # 'the cat the' against 'the cat sat on mat': num = (2, 1, 0, 0), den = (3, 2, 1, 1), brevity penalty exp(1 - 5/3);
    # bleu1 and bleu2 carry num_3 = num_4 = 0 at weight 0
    assert C.string_counts(["the cat the".split(" ")], ["the cat sat on mat".split(" ")]) == [2, 1, 0, 0, 3, 2, 1, 1, 3, 5]
    got, bp = f([2, 1, 0, 0, 3, 2, 1, 1, 3, 5]), math.exp(-2.0 / 3.0)
    assert _close(got["bleu1"], bp * 2 / 3) and _close(got["bleu2"], bp * math.sqrt(1 / 3))
    assert _close(got["bleu3"], bp * (2 / 3) ** .33 * .5 ** .33 * FMIN ** .33)
    assert _close(got["bleu4"], bp * (2 / 3) ** .25 * .5 ** .25 * FMIN ** .5) and 0.0 < got["bleu4"] < 1e-150
    # a hypothesis side longer than the reference side: no penalty; and hyp_len == 0: the penalty is 0
    got = f([4, 2, 1, 0, 5, 4, 3, 2, 5, 4])
    assert _close(got["bleu1"], 0.8) and _close(got["bleu2"], math.sqrt(0.8 * 0.5))
    assert f([1, 0, 0, 0, 1, 1, 1, 1, 0, 1])["bleu1"] == 0.0
    assert _close(f([3, 2, 1, 1, 3, 2, 1, 1, 3, 3])["bleu4"], 1.0)                  # equal lengths: exp(1 - 1) = 1
    with pytest.raises(ValueError):
        f([1, 2, 3])


def test_bleu_from_counters_equals_nltk():
    bleu_score = pytest.importorskip("nltk.translate.bleu_score")
    hyps = [C.hyp_words(r) for c in SMALL for r in c["ids"]]
    refs = [c["refs"][min(max(int(d), 0), len(c["refs"]) - 1)].split(" ") for c in SMALL for d in c["idx"]]
    got = RE.bleu_from_counters(C.string_counts(hyps, refs))
    for name, w in RE.WEIGHTS.items():
        want = bleu_score.corpus_bleu([[r] for r in refs], hyps, weights=w)
        assert _close(got[name], float(want)), (name, got[name], want)
