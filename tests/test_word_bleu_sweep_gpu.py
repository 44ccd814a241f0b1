"""Sweep of csrc/mv_bleu.hip on the MI355X against the string reference of tests/bleu_cases.py.  Every output is an integer, so the
comparison is exact: mv_bleu_words' keys against the host-keyed words of the reference's strings (and zeros behind them), mv_bleu_counts'
counters against collections.Counter on those strings.  The library is called through the C ABI with buffers of the test's own: every
output sits between guard elements in a sentinel-filled buffer (test_vqa_bank_sweep_gpu.Guarded); after the call the guards still hold
the sentinel.  test_bleu_cases_cpu.py shows that the cases reach what they are named after and that the comparison catches the planted
defects.  Twenty cases, two small launches each and three passes: a few seconds in all."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from medvill_amd import hip_ops as ops              # noqa: E402
from medvill_amd import report_eval as RE           # noqa: E402
import bleu_cases as C                              # noqa: E402
from test_vqa_bank_sweep_gpu import Guarded, call, dev      # noqa: E402

pytestmark = pytest.mark.gpu
CASES = C.cases()


@pytest.fixture(scope="module")
def tables():
    tb = RE.word_tables(C.TOKENS)
    return {k: tb[k].cuda() for k in ("tok_key", "tail_key", "tail_pow")}, tb["empty_key"]


def _words(ids_d, ld, n, T, tables):
    tb, empty = tables
    out = Guarded(dict(word_key=(torch.int64, n * T), n_words=(torch.int32, n)))
    call("mv_bleu_words", ids_d.data_ptr(), ld, n, T, tb["tok_key"].data_ptr(), tb["tail_key"].data_ptr(), tb["tail_pow"].data_ptr(), C.V,
         C.SEP, C.PAD, empty, out.p("word_key"), out.p("n_words"))
    torch.cuda.synchronize()
    return out


def _counts(hyp, T, n, ref_key, ref_n, idx_d, out):
    call("mv_bleu_counts", hyp.p("word_key"), T, hyp.p("n_words"), n, ref_key.data_ptr(), int(ref_key.shape[1]), ref_n.data_ptr(),
         int(ref_key.shape[0]), idx_d.data_ptr(), out.p("counters"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_both_kernels_equal_the_string_reference(case, tables):
    ids = case["ids"]
    n, T = ids.shape
    words = [C.hyp_words(r) for r in ids]
    want_key = np.zeros((n, T), np.uint64)
    for i, w in enumerate(words):
        want_key[i, :len(w)] = [C.key_of(x) for x in w]
    want_key, want_n = want_key.view(np.int64), np.array([len(w) for w in words], np.int32)
    hyp = _words(dev(ids), T, n, T, tables)
    hyp.check("word_key", want_key)
    hyp.check("n_words", want_n)
    wide = np.full((n, T + 3), C.ID["the"], np.int64)                       # rows of stride T + 3 whose padding holds a word
    wide[:, :T] = ids
    strided = _words(dev(wide), T + 3, n, T, tables)
    strided.check("word_key", want_key)
    strided.check("n_words", want_n)

    rk, rn = RE.text_keys(case["refs"])
    rk, rn, idx_d = rk.cuda(), rn.cuda(), dev(case["idx"])
    want = C.case_string_counts(case)
    runs = []
    for _ in range(2):                                                      # twice into a zeroed block: the same bits
        out = Guarded(dict(counters=(torch.int64, C.NCOUNT)))
        out.t("counters").zero_()
        _counts(hyp, T, n, rk, rn, idx_d, out)
        out.check("counters", np.array(want, np.int64))
        runs.append(out)
    assert torch.equal(runs[0].flat["counters"], runs[1].flat["counters"])
    _counts(hyp, T, n, rk, rn, idx_d, runs[1])                              # accumulated, not overwritten: two launches sum
    runs[1].check("counters", 2 * np.array(want, np.int64))


def test_wrappers_equal_the_string_reference(tables):
    tb, empty = tables
    case = next(c for c in CASES if c["name"] == "idx_repeats_and_leaves_the_bank")
    wide = torch.full((6, 11), C.ID["cat"], dtype=torch.int64, device="cuda")
    wide[:, :8] = dev(case["ids"])
    hk, hn = ops.bleu_words(wide[:, :8], tb["tok_key"], tb["tail_key"], tb["tail_pow"], C.SEP, C.PAD, empty)      # a strided view
    assert hn.tolist() == [len(C.hyp_words(r)) for r in case["ids"]] and hk.dtype == torch.int64 and tuple(hk.shape) == (6, 8)
    rk, rn = RE.text_keys(case["refs"])
    args = (hk, hn, rk.cuda(), rn.cuda(), dev(case["idx"]))
    counters = ops.bleu_counts(*args)
    counters = ops.bleu_counts(*args, counters=counters)
    want = C.case_string_counts(case)
    assert counters.dtype == torch.int64 and counters.tolist() == [2 * v for v in want]
    got = RE.bleu_from_counters(counters.cpu())
    assert got == RE.bleu_from_counters(want) and 0.0 < got["bleu2"] < got["bleu1"] < 1.0
    with pytest.raises(TypeError):
        ops.bleu_counts(*args, counters=torch.zeros(7, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        ops.bleu_counts(hk, hn, rk.cuda(), rn.cuda(), dev(case["idx"]).to(torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bleu_words(wide.cpu(), tb["tok_key"], tb["tail_key"], tb["tail_pow"], C.SEP, C.PAD, empty)
