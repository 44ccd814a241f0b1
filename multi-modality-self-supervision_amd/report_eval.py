"""Corpus BLEU-1..4 of generated reports: the last stage of the reference's report-generation evaluation
(Downstream_task/report_generation_and_vqa/sc/generation_decode.py:480-498 with sc/bleu.py:16-64) -- cut the generated ids at the
first [SEP] / [PAD], merge the word pieces (detokenize, :97-104), join and split on ' ', and take nltk's corpus_bleu at four weightings
against gt_caption.split(' ').

    bank.set_vocab(tokens).set_references(gt_captions)         # data.ReportBank: once
    out = model.evaluate(bank, beam_size=4, max_len=128)       # CXRBertForReportFinetune / CXRBertForGeneration
    out["bleu1"], ..., out["bleu4"]

Words are compared on the device through 64-bit keys (csrc/mv_bleu.hip): key(s) is the polynomial hash of s's UTF-8 bytes modulo 2^64
with the odd multiplier P, so that the key of a word assembled from word pieces follows from the pieces' keys,
key(a + b) = key(a) P^len(b) + key(b).  Equal keys are taken for equal words (DESIGN.md "8u" has the odds).  The score itself is
`bleu_from_counters` over ten integers, in float64 on the host.
"""
from __future__ import annotations

import math
import sys

import numpy as np
import torch

from . import hip_ops as ops

P = 0x9E3779B97F4A7C15                  # odd: multiplying by a power of it is a bijection modulo 2^64
_M = (1 << 64) - 1
WEIGHTS = {"bleu1": (1, 0, 0, 0), "bleu2": (0.5, 0.5, 0, 0), "bleu3": (0.33, 0.33, 0.33, 0), "bleu4": (0.25, 0.25, 0.25, 0.25)}      # bleu.py:50-53 (sic)
END_TOKENS = ("[SEP]", "[PAD]")         # generation_decode.py:485


def str_key(s: str) -> int:
    """The key of a string as an unsigned 64-bit integer: sum of byte_i P^(len - 1 - i) modulo 2^64; key('') = 0."""
    k = 0
    for b in s.encode("utf-8"):
        k = (k * P + b) & _M
    return k


def _i64(values) -> torch.Tensor:
    """Unsigned 64-bit integers -> the int64 tensor of the same bits."""
    return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64))


def word_tables(vocab_tokens) -> dict:
    """The tables mv_bleu_words composes words from, for the vocabulary id -> token string: tok_key, tail_key, tail_pow int64 [V] on
    the host (the bits of the unsigned keys) and empty_key.  tail_* describe tok[2:] of a token that starts with '##'; tail_pow is 0 for
    every other token.  An empty token or one that contains a space is refused: it would change the word count of the joined text."""
    tokens = list(vocab_tokens)
    if not tokens:
        raise ValueError("word_tables: an empty vocabulary")
    tok, tail, pw = [], [], []
    for i, t in enumerate(tokens):
        if not isinstance(t, str) or t == "" or " " in t:
            raise ValueError(f"word_tables: token {i} ({t!r}) is empty or contains a space")
        cont = t.startswith("##")
        tok.append(str_key(t))
        tail.append(str_key(t[2:]) if cont else 0)
        pw.append(pow(P, len(t[2:].encode("utf-8")), 1 << 64) if cont else 0)
    return dict(tok_key=_i64(tok), tail_key=_i64(tail), tail_pow=_i64(pw), empty_key=str_key(""))


def text_keys(texts):
    """The keys of text.split(' ') per report, exactly: the empty words of double, leading or trailing spaces are kept and nothing is
    lower-cased -> (keys int64 [n, W] padded with 0, counts int32 [n]) on the host, W the longest report's word count."""
    rows = [[str_key(w) for w in t.split(" ")] for t in texts]
    if not rows:
        raise ValueError("text_keys: no texts")
    W = max(len(r) for r in rows)
    keys = np.zeros((len(rows), W), dtype=np.uint64)
    for i, r in enumerate(rows):
        keys[i, :len(r)] = r
    return torch.from_numpy(keys.view(np.int64)), torch.tensor([len(r) for r in rows], dtype=torch.int32)


def decode_text(ids, vocab_tokens) -> list:
    """The reference's gen_caption strings (generation_decode.py:482-490) of ids [n, T]: the tokens before the first [SEP] / [PAD], word
    pieces merged as detokenize does, joined with ' '."""
    tokens = list(vocab_tokens)
    out = []
    for row in torch.as_tensor(ids).cpu().tolist():
        words = []
        for i in row:
            t = tokens[i]
            if t in END_TOKENS:
                break
            if t.startswith("##") and words:
                words[-1] += t[2:]
            else:
                words.append(t)
        out.append(" ".join(words))
    return out


def bleu_from_counters(counters) -> dict:
    """mv_bleu_counts' ten integers {num_1..4, den_1..4, hyp_len, ref_len} -> dict(bleu1..bleu4) in float64: nltk's corpus_bleu without
    smoothing at the reference's four weightings.  p_o = num_o / den_o over the corpus sums; a zero num_o is replaced by
    sys.float_info.min; the brevity penalty is 1 for hyp_len > ref_len, 0 for hyp_len == 0, else exp(1 - ref_len / hyp_len); the
    score is 0 when num_1 == 0."""
    c = [int(v) for v in torch.as_tensor(counters).reshape(-1).tolist()]
    if len(c) != ops.BLEU_NCOUNT:
        raise ValueError(f"bleu_from_counters: {ops.BLEU_NCOUNT} counters")
    num, den, hyp_len, ref_len = c[0:4], c[4:8], c[8], c[9]
    if num[0] == 0:
        return {k: 0.0 for k in WEIGHTS}
    bp = 1.0 if hyp_len > ref_len else 0.0 if hyp_len == 0 else math.exp(1.0 - ref_len / hyp_len)
    p = [n / d if n else sys.float_info.min for n, d in zip(num, den)]
    return {k: bp * math.exp(math.fsum(w_ * math.log(p_) for w_, p_ in zip(w, p))) for k, w in WEIGHTS.items()}


@torch.no_grad()
def evaluate(model, bank, idx=None, batch_size=64, **generate_kwargs) -> dict:
    """The reference's BLEU evaluation over the items `idx` of a data.ReportBank (None: every item, in order) that holds a vocabulary
    and references (set_vocab, set_references); a last partial batch is allowed.  Per batch the items' region features and positions
    are taken from the bank and handed to model.generate with the caller's beam_size / max_len / min_len / length_penalty / no_repeat_*
    arguments; the ids go into one [n, max_len] device buffer.  Then ONE mv_bleu_words launch, ONE mv_bleu_counts launch and ONE
    read-back of the ten counters.  `generate` itself is unchanged: its early-exit checks read a flag back every eight steps, and a
    beam search's finalize runs on the host -- the single read-back is that of the metric, not of the whole call.
    -> dict(bleu1..bleu4 (bleu_from_counters), counters int64 [10] on the host, ids int64 [n, max_len] on the device, n).
    The engine's training / keep-activations / dropout-counter state is restored (by generate; nothing else here touches it).  idx on the host is checked against the bank; idx
    on the device (int32) is clamped into it.  Refused: a bank without vocabulary or references, a vocabulary of another size than
    the model's, forced_ids, return_traces, max_len > 1024."""
    if generate_kwargs.get("forced_ids") is not None or generate_kwargs.get("return_traces"):
        raise ValueError("evaluate: forced_ids / return_traces belong to generate(); the evaluation decodes freely and keeps the ids")
    bs = int(batch_size)
    if bs < 1:
        raise ValueError("batch_size >= 1")
    bert = model.bert
    eng = bert.engine
    bank.check_eval(bert.cfg.vocab_size)
    n_items = bank.n_texts
    if torch.is_tensor(idx) and idx.device.type != "cpu":
        if idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() == 0:
            raise TypeError("idx on the device: non-empty int32 [n]")
        dev_idx = idx.contiguous()
    else:
        dev_idx = bank._index_list(torch.arange(n_items) if idx is None else idx, n_items, "items").to(torch.int32).to(eng.device)
    items = dev_idx.to(torch.int64).clamp_(0, n_items - 1)
    n = int(dev_idx.numel())
    max_len = int(generate_kwargs.get("max_len", 254))
    if max_len > ops.BLEU_MAX_WORDS:
        raise ValueError(f"evaluate: max_len {max_len} is past the {ops.BLEU_MAX_WORDS} tokens per row mv_bleu_words takes")
    v = bank.vocab
    ids = torch.empty((n, max_len), dtype=torch.int64, device=eng.device)
    for s in range(0, n, bs):
        take = items[s:s + bs]
        cls_tok, sep_tok = bank._tokens(int(take.numel()))
        ids[s:s + bs] = model.generate(cls_tok, (bank.img_feats.index_select(0, take), bank.img_pos.index_select(0, take)), sep_tok,
                                       **generate_kwargs)[0]
    hyp_key, hyp_n = ops.bleu_words(ids, v["tok_key"], v["tail_key"], v["tail_pow"], v["sep_id"], v["pad_id"], v["empty_key"])
    host = ops.bleu_counts(hyp_key, hyp_n, bank.ref_key, bank.ref_n, dev_idx).cpu()               # the one read-back of the metric
    out = bleu_from_counters(host)
    out.update(counters=host, ids=ids, n=n)
    return out
