"""Every reject of mv_bleu_words and mv_bleu_counts, in the manner of tests/test_ngram_abi_rejects.py: the entry points validate their
arguments BEFORE they touch the HIP runtime, so this runs without a GPU.  No call below may reach a launch."""
import pytest

import medvill_amd  # noqa: F401
from medvill_amd import _lib
from medvill_amd import hip_ops as ops

E_ARG, E_SHAPE = -1, -2
P = 0x1000          # a non-null address that is never dereferenced
CAP_T, CAP_V, CAP_N = 1024, 1 << 20, 1 << 20


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_caps_are_the_wrappers(lib):
    assert (ops.BLEU_MAX_WORDS, ops.BLEU_MAX_VOCAB, ops.BLEU_MAX_ROWS, ops.BLEU_NCOUNT) == (CAP_T, CAP_V, CAP_N, 10)


def test_bleu_words_rejects(lib):
    def bw(**k):
        return lib.mv_bleu_words(k.get("ids", P), k.get("ld", 16), k.get("n", 4), k.get("T", 16), k.get("tok", P), k.get("tail", P),
                                 k.get("pow", P), k.get("V", 40), 3, 0, 0, k.get("out", P), k.get("cnt", P), None)
    for name in ("ids", "tok", "tail", "pow", "out", "cnt"):
        assert bw(**{name: None}) == E_ARG, name
    assert bw(n=0) == E_ARG and bw(n=-1) == E_ARG and bw(T=0) == E_ARG and bw(V=0) == E_ARG and bw(T=-3, ld=-3) == E_ARG
    assert bw(ld=15) == E_ARG                                                           # ld < T
    assert bw(T=CAP_T + 1, ld=CAP_T + 1) == E_SHAPE and bw(V=CAP_V + 1) == E_SHAPE and bw(n=CAP_N + 1) == E_SHAPE


def test_bleu_counts_rejects(lib):
    def bc(**k):
        return lib.mv_bleu_counts(k.get("hyp", P), k.get("Th", 16), k.get("hyp_n", P), k.get("n", 4), k.get("ref", P), k.get("Tr", 12),
                                  k.get("ref_n", P), k.get("n_items", 3), k.get("idx", P), k.get("counters", P), None)
    for name in ("hyp", "hyp_n", "ref", "ref_n", "idx", "counters"):
        assert bc(**{name: None}) == E_ARG, name
    for name in ("Th", "n", "Tr", "n_items"):
        assert bc(**{name: 0}) == E_ARG and bc(**{name: -2}) == E_ARG, name
    assert bc(Th=CAP_T + 1) == E_SHAPE and bc(Tr=CAP_T + 1) == E_SHAPE and bc(n=CAP_N + 1) == E_SHAPE
