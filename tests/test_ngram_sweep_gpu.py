"""Sweep of the n-gram blocking kernels (csrc/mv_decode.hip: mv_ngram_ban, mv_logprob_topk_banned) over every case of
tests/ngram_cases.py (GPU).  tests/test_ngram_cases_cpu.py counts the branches the cases reach.

* mv_ngram_ban: the new histories, the ban lists and their counts are integers and compared exactly with the plain-Python rule; the
  columns behind len / nban and the guard rows around every output keep their sentinels; the inputs come back untouched.
* mv_logprob_topk_banned: every emitted value against the fp64 reference within the bound decode_cases.py derives for
  mv_logprob_topk on the same logits, plus half an f32 ulp at 10000 for a banned column's one extra rounding; -10000 exactly for the
  penalised EOS column, -inf exactly; the index list exactly wherever the reference's margins exceed the bounds (ngram_cases.tkb_excused
  names the few entries where they do not; an exact tie goes to the lower column and is asserted); with a null or empty ban list
  vals, idx and lse are bit-equal to mv_logprob_topk's.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import decode_cases as D                      # noqa: E402
import ngram_cases as C                       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _guarded(rows, ld, fill):
    """int32 [rows, ld] inside an allocation with guard rows before and after, everything pre-filled"""
    flat = torch.full(((rows + 2 * C.GUARD_ROWS) * ld + 8,), fill, dtype=torch.int32, device=DEV)
    return flat, flat[C.GUARD_ROWS * ld:(C.GUARD_ROWS + rows) * ld].view(rows, ld)


@pytest.mark.parametrize("cfg", C.nb_cases(), ids=lambda c: f"{c['seed']}-n{c['n']}-L{c['L']}-R{c['R']}-{c['parent']}")
def test_ngram_ban_cases(cfg):
    R, L, n, ld_h, ld_ban = cfg["R"], cfg["L"], cfg["n"], cfg["ld_h"], cfg["ld_ban"]
    info = dict(cfg, branches=C.nb_branches(cfg))
    i = C.nb_inputs(cfg)
    want = C.nb_expected(cfg, i)
    hist_in = i["hist_in"].to(DEV)
    parent = i["parent"].to(DEV) if i["parent"] is not None else None
    y = i["y"].to(DEV)
    ignore = i["ignore"].to(DEV) if i["ignore"] is not None else None
    keep = [t.clone() for t in (hist_in, y)]
    out_flat, hist_out = _guarded(R, ld_h, C.HIST_SENTINEL)
    ban_flat, ban = _guarded(R, ld_ban, C.BAN_SENTINEL)
    nban_flat, nban = _guarded(1, R, C.NBAN_SENTINEL)
    ops.ngram_ban(hist_in, hist_out, y, L - 1, n, ban, nban[0], parent=parent, ignore=ignore, R=R)
    torch.cuda.synchronize()
    assert torch.equal(hist_in, keep[0]) and torch.equal(y, keep[1]), info
    got_h, got_b, got_n = hist_out.cpu(), ban.cpu(), nban[0].cpu()
    assert got_h[:, :L].tolist() == i["seqs"], info
    assert bool((got_h[:, L:] == C.HIST_SENTINEL).all()), info
    assert got_n.tolist() == [len(w) for w in want], (info, got_n.tolist(), want)
    for r in range(R):
        assert got_b[r, :len(want[r])].tolist() == want[r], (info, r)
        assert bool((got_b[r, len(want[r]):] == C.BAN_SENTINEL).all()), (info, r)
    for flat, rows, ld, fill in ((out_flat, R, ld_h, C.HIST_SENTINEL), (ban_flat, R, ld_ban, C.BAN_SENTINEL), (nban_flat, 1, R, C.NBAN_SENTINEL)):
        g = C.GUARD_ROWS * ld
        assert bool((flat[:g] == fill).all()) and bool((flat[g + rows * ld:] == fill).all()), info


@pytest.mark.parametrize("cfg", C.tkb_cases(), ids=lambda c: f"{c['seed']}-V{c['V']}-k{c['k']}-{c['ban_mode']}-{c['eos_mode']}")
def test_logprob_topk_banned_cases(cfg):
    V, k, ld = cfg["V"], cfg["k"], cfg["ld"]
    info = dict(cfg, branches=C.tkb_branches(cfg))
    x_c, ban_c, nban_c = C.tkb_inputs(cfg)
    R = x_c.shape[0]
    eos = D.tk_eos(cfg)
    x = x_c.to(DEV)
    ban = ban_c.to(DEV) if ban_c is not None else None
    nban = nban_c.to(DEV) if nban_c is not None else None
    before = [t.clone() for t in (x, ban, nban) if t is not None]
    g = D.TK_GUARD_ROWS
    vals = torch.full((R + 2 * g, k), float("nan"), dtype=torch.float32, device=DEV)
    idx = torch.full((R + 2 * g, k), D.TK_IDX_SENTINEL, dtype=torch.int64, device=DEV)
    lse = torch.full((R + 2 * g,), float("nan"), dtype=torch.float32, device=DEV) if cfg["lse_out"] else None
    ops.logprob_topk_banned(x, k, R=R, V=V, ld=ld, eos_penalty_id=eos, ban=ban, nban=nban, vals=vals[g:g + R], idx=idx[g:g + R],
                            lse=lse[g:g + R] if lse is not None else None)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [t for t in (x, ban, nban) if t is not None])), info
    assert bool(torch.isnan(vals[:g]).all()) and bool(torch.isnan(vals[g + R:]).all()), info
    assert bool((idx[:g] == D.TK_IDX_SENTINEL).all()) and bool((idx[g + R:] == D.TK_IDX_SENTINEL).all()), info
    assert lse is None or (bool(torch.isnan(lse[:g]).all()) and bool(torch.isnan(lse[g + R:]).all())), info
    got_v, got_i = vals[g:g + R], idx[g:g + R]
    assert not torch.isnan(got_v).any() and bool(((got_i >= 0) & (got_i < V)).all()), info
    assert all(len(set(row)) == k for row in got_i.tolist()), info                      # no column twice

    x64 = x[:, :V].double()
    ref = C.tkb_reference(x64.cpu(), k, eos, ban_c, nban_c)
    ref = {n_: t.to(DEV) for n_, t in ref.items()}
    plain_v, plain_i, _ = D.tk_reference(x64, k, eos)
    lp_cpu, lse_cpu = D.tk_f32_cpu(x_c[:, :V], k, eos)
    tol = D.case_tol(D.TK_TOL, lp_cpu.to(DEV).gather(1, plain_i), plain_v)               # as the sweep of mv_logprob_topk derives it
    # the order
    excused = C.tkb_excused(ref, C.tkb_bound(ref, tol))
    same = got_i == ref["idx"]
    print(f"DEV tkb seed {cfg['seed']} excused {int(excused.sum())} of {excused.numel()} entries, {int((~same).sum())} differ")
    assert bool((same | excused).all()), (info, got_i.tolist(), ref["idx"].tolist())
    # the values, each against the reference value of the column it names
    want = ref["lp"].gather(1, got_i)
    bound = C.tkb_bound(ref, tol, got_i)
    ninf = torch.isinf(want)
    pen = (got_i == eos) if 0 <= eos < V else torch.zeros_like(ninf)
    assert bool((got_v[ninf] == -math.inf).all()), info
    assert bool((got_v[pen] == C.BAN_PENALTY).all()) and bool((want[pen] == C.BAN_PENALTY).all()), info
    rest = ~ninf
    ratio = float(((got_v[rest].double() - want[rest]).abs() / bound[rest]).max()) if bool(rest.any()) else 0.0
    print(f"DEV tkb values seed {cfg['seed']} error/bound {ratio:.3e} tolerance {tol:.3e}")
    assert ratio <= 1.0, (info, ratio)
    if lse is not None:
        ltol = D.case_tol(D.TK_TOL, lse_cpu.to(DEV), ref["lse"])
        lerr = float((lse[g:g + R].double() - ref["lse"]).abs().max())
        assert lerr <= ltol, (info, lerr, ltol)
    # no ban in force: the bits of mv_logprob_topk
    if ban_c is None or int(nban_c.max()) == 0:
        pv, pi = ops.logprob_topk(x, k, R=R, V=V, ld=ld, eos_penalty_id=eos)
        pl = torch.empty(R, dtype=torch.float32, device=DEV)
        ops.logprob_topk(x, k, R=R, V=V, ld=ld, eos_penalty_id=eos, lse=pl)
        assert torch.equal(got_i, pi) and torch.equal(got_v.view(torch.int32), pv.view(torch.int32)), info
        assert lse is None or torch.equal(lse[g:g + R].view(torch.int32), pl.view(torch.int32)), info
