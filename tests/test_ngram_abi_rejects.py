"""Every reject of mv_ngram_ban and mv_logprob_topk_banned, in the manner of tests/test_abi_rejects.py: the entry points validate their
arguments BEFORE they touch the HIP runtime, so this runs without a GPU.  No call below may reach a launch."""
import pytest

import medvill_amd  # noqa: F401
from medvill_amd import _lib

import ngram_cases as C

E_ARG, E_SHAPE = -1, -2
P = 0x1000          # non-null addresses that are never dereferenced
Q = 0x100000


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_ngram_ban_rejects(lib):
    def nb(**k):
        return lib.mv_ngram_ban(k.get("hin", P), k.get("hout", Q), k.get("ld_h", 64), k.get("parent", None), k.get("y", P), k.get("R", 4),
                                k.get("len", 10), k.get("n", 3), k.get("ign", None), k.get("n_ign", 0), k.get("ban", P), k.get("ld_ban", 64),
                                k.get("nban", P), None)
    assert nb(hin=None) == E_ARG and nb(hout=None) == E_ARG and nb(y=None) == E_ARG and nb(ban=None) == E_ARG and nb(nban=None) == E_ARG
    assert nb(R=0) == E_ARG and nb(len=-1) == E_ARG and nb(n_ign=-1) == E_ARG and nb(ld_h=0) == E_ARG and nb(ld_ban=-1) == E_ARG
    assert nb(n_ign=3) == E_ARG                                                         # ignore ids announced but absent
    assert nb(n=C.NB_MIN_N - 1) == E_ARG and nb(n=C.NB_MAX_N + 1) == E_ARG and nb(n=0) == E_ARG
    # aliasing histories: the same buffer, and any overlap of the two [R, ld_h] extents
    assert nb(hout=P) == E_ARG
    assert nb(hout=P + 4 * (3 * 64 + 10)) == E_ARG and nb(hin=Q + 4 * 64, hout=Q) == E_ARG
    assert nb(len=63, ld_h=63) == E_SHAPE                                               # ld_h < len + 1
    assert nb(len=10, n=3, ld_ban=8) == E_SHAPE                                         # ld_ban < len + 2 - n
    assert nb(len=C.NB_MAX_LEN, ld_h=2048, ld_ban=2048) == E_SHAPE                      # len + 1 over the cap
    assert nb(ign=P, n_ign=C.NB_MAX_IGN + 1) == E_SHAPE                                 # ignore ids over the cap


def test_logprob_topk_banned_rejects(lib):
    def tk(**k):
        return lib.mv_logprob_topk_banned(k.get("x", P), k.get("ld", 40), k.get("R", 2), k.get("V", 40), k.get("k", 4), -1, k.get("ban", P),
                                          k.get("ld_ban", 8), k.get("nban", P), k.get("vals", P), k.get("idx", P), None, None)
    assert tk(x=None) == E_ARG and tk(vals=None) == E_ARG and tk(idx=None) == E_ARG and tk(R=0) == E_ARG and tk(k=0) == E_ARG and tk(ld=39) == E_ARG
    assert tk(nban=None) == E_ARG and tk(ld_ban=0) == E_ARG                             # a ban list without its counts / width
    assert tk(k=17) == E_SHAPE                                                          # k <= 16
    assert tk(k=5, V=4, ld=4) == E_SHAPE                                                # k <= V
    assert tk(V=C.TKB_MAX_V + 1, ld=C.TKB_MAX_V + 1) == E_SHAPE                         # V over the bitmap
    assert tk(V=C.TKB_MAX_V + 1, ld=C.TKB_MAX_V + 1, ban=None, nban=None) == E_SHAPE    # ... with or without a ban list
