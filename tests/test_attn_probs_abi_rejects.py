"""mv_attn_probs on the CPU: the symbol is exported and declared with the arity of its ctypes prototype, and every rejection of
include/medvill.h returns its code before anything is launched -- the output is a real, NaN-filled host buffer that must come back
untouched (a launcher that refuses writes nothing; a kernel could not write host memory anyway)."""
import ctypes
import os
import re

import numpy as np
import pytest

import medvill_amd  # noqa: F401
from medvill_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
F32, BF16, F16 = 0, 1, 2
P = 0x1000          # a non-null, 64-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbol_header_and_prototype_agree():
    hdr = open(os.path.join(ROOT, "include", "medvill.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+mv_attn_probs\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, "mv_attn_probs is not declared in include/medvill.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs == len(_lib.PROTOTYPES["mv_attn_probs"]) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mv_attn_probs") and hasattr(ctypes.CDLL(_lib.DBG_LIB_PATH), "mv_attn_probs")
    assert _lib.ABI_VERSION == 6 and "#define MV_ABI_VERSION 6" in hdr            # the entry is additive


def test_every_rejection_returns_before_any_launch(lib):
    def aligned(n, dt, fill):                # 64-byte aligned, whatever the allocator returns
        raw = np.empty(n * np.dtype(dt).itemsize + 64, dtype=np.uint8)
        a = raw[(-raw.ctypes.data) % 64:][:n * np.dtype(dt).itemsize].view(dt)
        a[...] = fill
        return a
    B, L, A = 2, 64, 2
    out = aligned(B * A * L * L, np.float32, np.nan)
    db = aligned(B * A * 2 * 64, np.uint32, 0x3C3C3C3C)
    before = (out.copy(), db.copy())
    po, pdb = out.ctypes.data, db.ctypes.data
    assert po % 16 == 0 and pdb % 64 == 0

    def f(dt=BF16, qkv=P, bits=P, info=P, lse=P, probs=None, odt=F32, B_=B, L_=L, A_=A, dh=64, p=0.0, db_=None, hm=0):
        return lib.mv_attn_probs(dt, qkv, bits, info, lse, po if probs is None else probs, odt, B_, L_, A_, dh, p, db_, hm, None)

    for hm in (0, 1):
        # null pointers and sizes that are not positive
        for k in ("qkv", "bits", "info", "lse"):
            assert f(**{k: None}, hm=hm) == E_ARG, k
        assert lib.mv_attn_probs(BF16, P, P, P, P, None, F32, B, L, A, 64, 0.0, None, hm, None) == E_ARG
        for k in ("B_", "L_", "A_", "dh"):
            assert f(**{k: 0}, hm=hm) == E_ARG and f(**{k: -3}, hm=hm) == E_ARG, k
        # encodings
        assert f(dt=3, hm=hm) == E_DTYPE and f(dt=-1, hm=hm) == E_DTYPE
        assert f(dt=BF16, odt=F16, hm=hm) == E_ARG and f(dt=F16, odt=BF16, hm=hm) == E_ARG and f(dt=F32, odt=BF16, hm=hm) == E_ARG
        assert f(odt=5, hm=hm) == E_ARG and f(odt=-1, hm=hm) == E_ARG
        # T = ceil(L / 64) > 64
        assert f(L_=64 * 64 + 1, hm=hm) == E_SHAPE and f(dt=F32, L_=5000, hm=hm) == E_SHAPE
        # head width: 64 on the 16-bit route, <= 128 on the f32 route
        for dt in (BF16, F16):
            assert f(dt=dt, dh=32, hm=hm) == E_SHAPE and f(dt=dt, dh=65, hm=hm) == E_SHAPE and f(dt=dt, dh=128, hm=hm) == E_SHAPE
        assert f(dt=F32, dh=129, hm=hm) == E_SHAPE and f(dt=F32, dh=256, hm=hm) == E_SHAPE
        # alignment of qkv and probs (16 bytes), on both routes
        for dt in (BF16, F16, F32):
            assert f(dt=dt, qkv=P + 8, hm=hm) == E_SHAPE and f(dt=dt, qkv=P + 2, hm=hm) == E_SHAPE
            assert f(dt=dt, probs=po + 8, hm=hm) == E_SHAPE and f(dt=dt, probs=po + 4, hm=hm) == E_SHAPE
        # dropout: the keep-bits are required and 64-byte aligned
        assert f(p=0.1, hm=hm) == E_ARG and f(dt=F32, p=0.1, hm=hm) == E_ARG
        assert f(p=1.0, db_=pdb, hm=hm) == E_ARG and f(p=1.5, db_=pdb, hm=hm) == E_ARG
        assert f(p=0.1, db_=pdb + 32, hm=hm) == E_SHAPE and f(p=0.1, db_=pdb + 4, hm=hm) == E_SHAPE
        # qkv of 2^31 bytes or more on the 16-bit route (read through a buffer descriptor)
        assert f(B_=1024, L_=4096, A_=12, hm=hm) == E_SHAPE
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((out, db), before))
