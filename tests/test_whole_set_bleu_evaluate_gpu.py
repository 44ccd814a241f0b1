"""CXRBertForReportFinetune.evaluate / CXRBertForGeneration.evaluate (report_eval.evaluate) on the MI355X: corpus BLEU-1..4 of the
reports generated for the items of a data.ReportBank, against the string reference of tests/bleu_cases.py applied to the ids the call
returns and the raw reference texts.  Everything compared is an integer or follows from integers by one host formula, so every
comparison is exact -- but the loss of a fit_step after the call, which test_report_bank_gpu.py's own bound for a step after generate()
covers (the step's f32 atomics rule out bitwise equality from the second step on).

The configuration is the smallest the package runs: one layer, 4 regions, a bank of 10 items at batch_size 4 (a partial last batch).
The vocabulary is hand-made with '##' pieces: 40 words behind BERT's 104 reserved slots, because the package's kernels place [UNK],
[CLS], [SEP] and [MASK] at ids 100-103 (mv_report_assemble writes 103 into a masked row), so a vocabulary of 40 ids in all could not
be embedded.  The decoder bias favours the 40 words, so that the generated reports share words with the references."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                     # noqa: E402
from medvill_amd import report_eval as RE    # noqa: E402
from oracle import cxrbert_oracle as O       # noqa: E402
import bleu_cases as C                       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORDS = ["the", "heart", "size", "is", "normal", ".", "no", "pleural", "eff", "##usion", "##s", "card", "##io", "##meg", "##aly", "lung",
         "are", "clear", "there", "acute", "disease", "##.", "mild", "at", "##ele", "##ct", "##asis", "left", "right", "base", "of", "and",
         "or", "pneumo", "##thorax", "seen", "stable", ",", "##ly", "x"]
VOCAB = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS
ID = {t: i for i, t in enumerate(VOCAB)}
CFG = O.OracleConfig(vocab_size=len(VOCAB), hidden=128, layers=1, heads=2, intermediate=512, max_pos=512)
N_REG, T_TXT, N_ITEMS, BATCH, MAX_LEN, MAX_PRED = 4, 14, 10, 4, 10, 4
PIECES = ["the heart size is normal .", "no pleural eff ##usion .", "card ##io ##meg ##aly is mild .", "the lung ##s are clear .",
          "there is no acute disease ##.", "mild at ##ele ##ct ##asis at the left base", "no pneumo ##thorax seen",
          "heart and lung ##s stable", "x", "the right lung is clear , the left is clear ."]
RAW = ["the heart size is normal.", "no pleural effusion .", "cardiomegaly is mild .", "the lungs are clear .", "there is no acute disease.",
       "Mild atelectasis at the  left base", "no pneumothorax seen", "heart and lungs stable", "x",
       "the right lung is clear , the left is clear ."]


def _cfg_dict():
    c = CFG
    return dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)


_P = {}


def _params():
    if not _P:
        _P.update(O.make_params(CFG, seed=3, scale=0.1))                     # weights large enough for the image to change the words
        _P["mlm.predictions.bias"][len(VOCAB) - len(WORDS):] += 3.0          # the hand-made words before the reserved slots ...
        _P["mlm.predictions.bias"][ID["[SEP]"]] += 2.0                       # ... and rows that end
    return _P


def _model(cls=None):
    m = (cls or mv.CXRBertForReportFinetune)(_cfg_dict(), dtype=torch.bfloat16, device=DEV, fwd_operand="bf16", grad_operand="bf16")
    m.bert.load_state_dict(_params(), strict=True)
    m.eval()
    return m


def _bank(m, vocab=True, refs=True):
    assert (ID["[PAD]"], ID["[UNK]"], ID["[CLS]"], ID["[SEP]"], ID["[MASK]"]) == (0, 100, 101, 102, 103) and len(PIECES) == len(RAW) == N_ITEMS
    ids = torch.zeros((N_ITEMS, T_TXT), dtype=torch.int64)
    lens = []
    for i, p in enumerate(PIECES):
        row = [ID[t] for t in p.split()] + [ID["[SEP]"]]
        ids[i, :len(row)] = torch.tensor(row)
        lens.append(len(row))
    g = torch.Generator().manual_seed(11)
    feats = torch.randn((N_ITEMS, N_REG, CFG.img_hidden), generator=g)
    pos = torch.tensor([7, 60, 131, 202]).view(1, N_REG).expand(N_ITEMS, N_REG).contiguous()
    bank = mv.data.ReportBank(m, max_pred=MAX_PRED)
    bank.add_reports(ids, torch.tensor(lens)).add_images((feats, pos))
    if vocab:
        bank.set_vocab(VOCAB)
    if refs:
        bank.set_references(RAW)
    return bank


def _tok(n, name):
    return torch.full((n, 1), ID[name], dtype=torch.int64, device=DEV)


def _want(ids, items):
    return C.string_counts([C.hyp_words(r, VOCAB) for r in ids.cpu().tolist()], [RAW[i].split(" ") for i in items])


@pytest.mark.parametrize("kw", [dict(), dict(beam_size=3, length_penalty=0.5, min_len=2), dict(beam_size=2, no_repeat_ngram_size=2)],
                         ids=["greedy", "beam3", "beam2-norepeat"])
def test_evaluate_equals_generate_and_the_string_reference(kw):
    m = _model()
    bank = _bank(m)
    out = m.evaluate(bank, batch_size=BATCH, max_len=MAX_LEN, **kw)
    ids = out["ids"]
    assert out["n"] == N_ITEMS and ids.is_cuda and ids.dtype == torch.int64 and tuple(ids.shape) == (N_ITEMS, MAX_LEN)
    for s in range(0, N_ITEMS, BATCH):                                     # batch by batch: what generate returns for the same items
        e = min(N_ITEMS, s + BATCH)
        got = m.generate(_tok(e - s, "[CLS]"), (bank.img_feats[s:e], bank.img_pos[s:e]), _tok(e - s, "[SEP]"), max_len=MAX_LEN, **kw)[0]
        assert torch.equal(ids[s:e], got), (s, ids[s:e].tolist(), got.tolist())
    assert len({tuple(r) for r in ids.tolist()}) > 1                       # the items differ: the order of the batches matters below
    want = _want(ids, range(N_ITEMS))
    counters = out["counters"]
    print(kw, "counters", counters.tolist(), "distinct rows", len({tuple(r) for r in ids.tolist()}), "texts", RE.decode_text(ids, VOCAB)[:3])
    assert not counters.is_cuda and counters.dtype == torch.int64 and counters.tolist() == want
    assert {k: out[k] for k in RE.WEIGHTS} == RE.bleu_from_counters(want)
    if not kw:                                                             # one shared function: the decoding-only holder gives the same
        g = _model(mv.CXRBertForGeneration)
        again = g.evaluate(bank, batch_size=BATCH, max_len=MAX_LEN)
        assert torch.equal(again["ids"], ids) and again["counters"].tolist() == want


def test_references_from_the_banks_own_rows_equal_their_decoded_texts():
    m = _model()
    bank = _bank(m, refs=False)
    bank.set_references(None)
    k0, n0 = bank.ref_key.cpu(), bank.ref_n.cpu()
    texts = RE.decode_text(bank.txt_ids, VOCAB)
    assert texts[1] == "no pleural effusion ." and texts[4] == "there is no acute disease."
    bank.set_references(texts)
    k1, n1 = bank.ref_key.cpu(), bank.ref_n.cpu()
    W = int(k1.shape[1])
    assert torch.equal(n0, n1) and tuple(k0.shape) == (N_ITEMS, T_TXT) and torch.equal(k0[:, :W], k1) and not bool(k0[:, W:].any())


def test_a_device_idx_and_a_host_idx_agree():
    m = _model()
    bank = _bank(m)
    idx = [3, 0, 9, 3, 7]
    host = m.evaluate(bank, idx, batch_size=2, max_len=MAX_LEN)
    on_dev = m.evaluate(bank, torch.tensor(idx, dtype=torch.int32, device=DEV), batch_size=2, max_len=MAX_LEN)
    assert host["n"] == on_dev["n"] == 5 and torch.equal(host["ids"], on_dev["ids"])
    assert host["counters"].tolist() == on_dev["counters"].tolist() == _want(host["ids"], idx)
    clamped = m.evaluate(bank, torch.tensor([-2, N_ITEMS + 2], dtype=torch.int32, device=DEV), max_len=MAX_LEN)
    inside = m.evaluate(bank, [0, N_ITEMS - 1], max_len=MAX_LEN)
    assert torch.equal(clamped["ids"], inside["ids"]) and clamped["counters"].tolist() == inside["counters"].tolist()
    with pytest.raises(IndexError):
        m.evaluate(bank, [0, N_ITEMS], max_len=MAX_LEN)


def _fit(evaluate_between):
    torch.manual_seed(0)
    m = _model()
    bank = _bank(m)
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    eng = m.bert.engine
    out = []
    for i in range(2):
        if evaluate_between and i == 1:
            state = (eng.training, eng.keep_acts, eng.drop_counter)
            m.evaluate(bank, batch_size=BATCH, max_len=MAX_LEN, beam_size=2)
            assert (eng.training, eng.keep_acts, eng.drop_counter) == state and m.training
        loss = m.fit_step(bank, [3, 0, 5, 3], opt, step=i, key=4)
        out.append((float(loss), dict(eng.S["drop_keys"]), eng.drop_counter))
    return out


def test_a_fit_step_after_evaluate_is_the_step_without_it():
    plain, between = _fit(False), _fit(True)
    for (l0, k0, c0), (l1, k1, c1) in zip(plain, between):
        assert k0 == k1 and c0 == c1                                       # the same dropout masks are drawn
    assert plain[0][0] == between[0][0]
    assert abs(plain[1][0] - between[1][0]) < 1e-3 * abs(plain[1][0])       # (test_report_bank_gpu.py's bound for a step after generate)


def test_refusals():
    m = _model()
    with pytest.raises(ValueError, match="vocabulary"):
        m.evaluate(_bank(m, vocab=False, refs=False), max_len=MAX_LEN)
    with pytest.raises(ValueError, match="references"):
        m.evaluate(_bank(m, refs=False), max_len=MAX_LEN)
    with pytest.raises(ValueError, match="set_vocab"):
        _bank(m, vocab=False, refs=False).set_references(None)
    bank = _bank(m)
    with pytest.raises(ValueError, match="forced_ids"):
        m.evaluate(bank, forced_ids=torch.zeros((N_ITEMS, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="return_traces"):
        m.evaluate(bank, beam_size=2, return_traces=True)
    with pytest.raises(ValueError, match="batch_size"):
        m.evaluate(bank, batch_size=0)
    with pytest.raises(ValueError, match="1024 tokens"):
        m.evaluate(bank, max_len=1025)
    with pytest.raises(ValueError, match="9 texts"):
        bank.set_references(RAW[:-1])
    with pytest.raises(ValueError, match="1025 words"):
        bank.set_references(RAW[:-1] + [" ".join(["x"] * 1025)])
    with pytest.raises(ValueError, match=r"\[SEP\]"):
        bank.set_vocab(["[PAD]", "a"])
    bank.set_vocab(VOCAB[:-1])
    with pytest.raises(ValueError, match="143 tokens"):
        m.evaluate(bank, max_len=MAX_LEN)
    empty = mv.data.ReportBank(m)
    with pytest.raises(ValueError):
        m.evaluate(empty)
