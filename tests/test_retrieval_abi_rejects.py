"""CPU-reachable half of csrc/mv_retrieval.hip's C ABI, in the manner of tests/test_abi_rejects.py: every entry validates its arguments
before it touches the HIP runtime, so each documented rejection (include/medvill.h) is exercised here without a GPU."""
import ctypes as C

import pytest

import medvill_amd  # noqa: F401
from medvill_amd import _lib

E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
F32, F16 = 0, 2
P = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below must return before a launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_pair_draws_and_negatives_reject(lib):
    dr = lambda **k: lib.mv_pair_draws(1, 2, k.get("B", 4), k.get("D", 1), k.get("out", P), None)
    assert dr(out=None) == E_ARG and dr(B=0) == E_ARG and dr(B=-1) == E_ARG and dr(D=0) == E_ARG
    assert dr(D=301) == E_SHAPE and dr(B=1 << 23) == E_SHAPE                               # 300 attempts; 32-bit hash counters
    ng = lambda **k: lib.mv_pair_negatives(k.get("idx", P), k.get("B", 4), k.get("n", 10), k.get("cls", None), 1, 2, k.get("draws", None),
                                           k.get("nd", 0), k.get("pairs", P), k.get("labels", P), None)
    assert ng(idx=None) == E_ARG and ng(pairs=None) == E_ARG and ng(labels=None) == E_ARG
    assert ng(B=0) == E_ARG and ng(B=-3) == E_ARG
    assert ng(n=1) == E_ARG and ng(n=0) == E_ARG and ng(n=-5) == E_ARG                     # a negative needs another item
    assert ng(draws=P, nd=0) == E_ARG and ng(draws=P, nd=-1) == E_ARG
    assert ng(B=1 << 23) == E_SHAPE


def test_pair_assemble_rejects(lib):
    def asm(**k):
        return lib.mv_pair_assemble(k.get("ids", P), k.get("len", P), k.get("Ti", 5), k.get("img", P), k.get("dt", F16), k.get("Ii", 4),
                                    k.get("ipos", None), k.get("pairs", P), k.get("R", 3), k.get("N", 3), k.get("S", 5), k.get("F", 8),
                                    k.get("txt", P), k.get("seg", P), k.get("n_ids", P), k.get("desc", P), k.get("feats", P),
                                    k.get("pos", None), None)
    for name in ("ids", "len", "img", "pairs", "txt", "seg", "n_ids", "desc", "feats"):
        assert asm(**{name: None}) == E_ARG, name
    for name in ("Ti", "Ii", "R", "N", "S", "F"):
        assert asm(**{name: 0}) == E_ARG and asm(**{name: -2}) == E_ARG, name
    assert asm(ipos=P) == E_ARG and asm(pos=P) == E_ARG                                    # positions: bank and output together
    assert asm(dt=3) == E_DTYPE and asm(dt=-1) == E_DTYPE
    assert asm(N=1 << 16, F=1 << 16) == E_SHAPE


def test_rank_groups_rejects(lib):
    ks = (C.c_int * 9)(1, 5, 10, 20, 30, 40, 50, 60, 70)
    kp = C.cast(ks, C.c_void_p)

    def rk(**k):
        return lib.mv_rank_groups(k.get("logits", P), k.get("labels", P), k.get("G", 2), k.get("C", 6), k.get("ks", kp), k.get("nk", 3),
                                  k.get("p", P), k.get("pos", P), k.get("rank", P), k.get("cnt", P), None)
    for name in ("logits", "labels", "p", "pos", "rank", "cnt"):
        assert rk(**{name: None}) == E_ARG, name
    assert rk(G=0) == E_ARG and rk(G=-1) == E_ARG
    assert rk(C=0) == E_ARG and rk(C=-4) == E_ARG                                          # C < 1
    assert rk(nk=9) == E_ARG and rk(nk=-1) == E_ARG and rk(ks=None) == E_ARG               # more than 8 cut-offs
    bad = (C.c_int * 3)(1, 0, 10)
    assert rk(ks=C.cast(bad, C.c_void_p)) == E_ARG                                         # a cut-off <= 0
    assert rk(G=1 << 20, C=1 << 12) == E_SHAPE
