"""Sweep of csrc/mv_clf_bank.hip on the MI355X against the numpy restatements of tests/clf_bank_cases.py.  Every output of the two entry
points is an integer, a copied bit pattern or an exact 0.0 / 1.0, so the comparison is exact (the target as f32 bit patterns, the
counters as integers, also after two accumulating launches into one block).  The library is called through the C ABI with buffers of the
test's own: every output sits between guard elements in a buffer pre-filled with a sentinel; after the call the elements the contract
writes hold the restatement's values and the guards still hold the sentinel.  test_clf_bank_cases_cpu.py shows that the case set reaches
every branch of the launcher but the capped grid (which the VQA sweep holds for the shared header) and that this comparison catches the
planted defects.

The file is ONE test item that walks every case (a hundred launches, seconds in all): all of them check one property, kernel ==
restatement.  A case that misses its comparison does not end the walk; the test fails at the end with the name and the assertion of
every case that missed.  Any other error (a HIP error among them) ends it at once."""
import os
import sys
import traceback

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from medvill_amd import hip_ops as ops        # noqa: E402
import clf_bank_cases as C                    # noqa: E402
from test_vqa_bank_sweep_gpu import DT, Guarded, call, dev      # noqa: E402

pytestmark = pytest.mark.gpu


def _bank_on_device(bank, dt):
    d = {k: dev(bank[k]) for k in ("txt_ids", "txt_len", "s_img", "lab_bits", "img_pos")}
    d["img_feats"] = dev(bank["img_feats"]).to(dt).contiguous()
    return d


def _assemble(bd, idx_d, fam_d, B, N, T, F, Cn, dt, guard):
    specs = dict(input_txt=(torch.int64, B * T), segment=(torch.int64, B * T), desc=(torch.int32, 3 * B), feats=(dt, B * N * F),
                 pos=(torch.int64, B * N), target=(torch.float32, B * Cn))
    out = Guarded(specs, guard)
    call("mv_clf_assemble", bd["txt_ids"].data_ptr(), bd["txt_len"].data_ptr(), bd["s_img"].data_ptr(), bd["lab_bits"].data_ptr(),
         int(bd["txt_ids"].shape[0]), bd["img_feats"].data_ptr(), ops.L.dt_of(bd["img_feats"]), bd["img_pos"].data_ptr(),
         int(bd["img_feats"].shape[0]), idx_d.data_ptr(), None if fam_d is None else fam_d.data_ptr(), B, N, T, F, Cn, out.p("input_txt"),
         out.p("segment"), out.p("desc"), out.p("feats"), out.p("pos"), out.p("target"))
    torch.cuda.synchronize()
    return out


def _sweep_id(c):
    return "B{}-C{}-T{}-NF{}-{}{}".format(c[0], c[1], c[2], c[3] * c[4], c[5], "-odd" if c[7] == C.GUARD_ODD else "")


def _check_assemble(case):
    B, Cn, T, N, F, dtn, fam, guard = case
    bank = C.sweep_bank(case)
    idx = C.batch_idx(bank, B, seed=B + T)
    g = np.random.default_rng(B + Cn)
    family = None if fam is None else g.choice([C.FAMILY_S2S, C.FAMILY_BAR, C.FAMILY_1D], B).astype(np.int32)
    ref = C.assemble(bank, idx, Cn, family)
    idx_d, fam_d = dev(idx), None if family is None else dev(family)
    for dt in DT.values():                                                 # every case in f32 / bf16 / f16 (its own encoding first)
        bd = _bank_on_device(bank, dt)
        runs = [_assemble(bd, idx_d, fam_d, B, N, T, F, Cn, dt, guard) for _ in range(2 if dt == DT[dtn] else 1)]
        for out in runs:
            for k in ("input_txt", "segment", "desc", "pos", "target"):
                out.check(k, ref[k])
            out.check("feats", torch.from_numpy(ref["feats"]).to(dt))       # the bank's values are exact in every encoding: a copy
        for k in runs[0].flat:                                             # two runs: bitwise equal, guards included
            assert torch.equal(runs[0].flat[k].view(torch.uint8), runs[-1].flat[k].view(torch.uint8)), k


def _counts(probs_d, ld, idx_d, bits_d, n, n_items, Cn, out):
    call("mv_clf_counts", probs_d.data_ptr(), ld, idx_d.data_ptr(), n, bits_d.data_ptr(), n_items, Cn, out.p("counters"))
    torch.cuda.synchronize()


def _check_counts(n, Cn):
    case = C.make_counts_case(n, Cn)
    want = C.counts(case["probs"], case["idx"], case["lab_bits"], Cn)
    assert int(want[Cn, C.N_POS] + want[Cn, C.N_NEG]) == n * Cn
    idx_d, bits_d, n_items = dev(case["idx"]), dev(case["lab_bits"]), len(case["hot"])
    out = Guarded(dict(counters=(torch.int64, (Cn + 1) * C.NCOUNT)))
    out.t("counters").zero_()
    _counts(dev(case["probs"]), Cn, idx_d, bits_d, n, n_items, Cn, out)
    out.check("counters", want)
    # a second launch into the same block, over rows of ld = C + 3 whose padding holds a probability that would count
    other = np.ascontiguousarray(np.roll(case["probs"], 1, axis=0))
    padded = np.full((n, Cn + 3), 0.75, np.float32)
    padded[:, :Cn] = other
    _counts(dev(padded), Cn + 3, idx_d, bits_d, n, n_items, Cn, out)
    out.check("counters", C.counts(other, case["idx"], case["lab_bits"], Cn, counters=want))


def _check_negative_zero_ties_with_zero():
    Cn, n = 2, 6
    probs = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 1.0], [-0.0, 0.5], [0.25, -0.0], [0.0, 0.0]], np.float32)
    hot = np.array([[1, 0], [0, 1], [1, 1], [0, 0], [0, 1], [1, 0]], bool)
    idx = np.arange(n, dtype=np.int32)
    bits = C.pack_bits(hot)
    want = C.counts(probs, idx, bits, Cn)
    assert want[0, C.EQ] == 6 and want[0, C.GT] == 0                        # class 0: every +0 / -0 pair is a tie
    out = Guarded(dict(counters=(torch.int64, (Cn + 1) * C.NCOUNT)))
    out.t("counters").zero_()
    _counts(dev(probs), Cn, dev(idx), dev(bits), n, n, Cn, out)
    out.check("counters", want)


def _check_wrappers_equal_the_direct_calls():
    case = C.SWEEP[1]
    B, Cn, T, N, F = case[:5]
    bank = C.sweep_bank(case)
    bd = _bank_on_device(bank, torch.float16)
    idx = C.batch_idx(bank, B, seed=3)
    fam = np.array([1, 2, 4], np.int32)
    got = ops.clf_assemble(bd["txt_ids"], bd["txt_len"], bd["s_img"], bd["lab_bits"], bd["img_feats"], bd["img_pos"], dev(idx), Cn,
                           family=dev(fam))
    ref = C.assemble(bank, idx, Cn, fam)
    for k in ("input_txt", "segment", "desc", "pos", "target"):
        assert got[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    assert np.array_equal(got["feats"].float().cpu().numpy(), ref["feats"])
    cc = C.make_counts_case(65, 33)
    args = (dev(cc["idx"]), dev(cc["lab_bits"]), 33)
    counters = ops.clf_counts(dev(cc["probs"]), *args)
    wide = torch.full((65, 40), 0.75, dtype=torch.float32, device="cuda")
    wide[:, :33] = dev(cc["probs"])
    counters = ops.clf_counts(wide[:, :33], *args, counters=counters)      # a strided view, accumulated
    want = C.counts(cc["probs"], cc["idx"], cc["lab_bits"], 33)
    assert counters.dtype == torch.int64 and tuple(counters.shape) == (34, 7) and np.array_equal(counters.cpu().numpy(), 2 * want)
    with pytest.raises(TypeError):
        ops.clf_counts(dev(cc["probs"]), *args, counters=torch.zeros(7, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        ops.clf_counts(dev(cc["probs"]), dev(cc["idx"]), dev(cc["lab_bits"][:, :1]), 33)


def _checks():
    for case in C.SWEEP:                                                   # mv_clf_assemble: every sweep case x f32 / bf16 / f16
        yield "assemble " + _sweep_id(case), _check_assemble, (case,)
    for n, Cn in C.COUNT_CASES:                                            # mv_clf_counts: n x C, two accumulating launches each
        yield f"counts n{n}-C{Cn}", _check_counts, (n, Cn)
    yield "counts -0 ties +0", _check_negative_zero_ties_with_zero, ()
    yield "wrappers", _check_wrappers_equal_the_direct_calls, ()


def test_both_kernels_equal_the_restatement_on_every_case():
    missed, n_run = [], 0
    for name, check, args in _checks():
        n_run += 1
        try:
            check(*args)
        except AssertionError:
            missed.append(f"---- {name}\n{traceback.format_exc(limit=-2)}")
    assert n_run == len(C.SWEEP) + len(C.COUNT_CASES) + 2
    assert not missed, f"{len(missed)} of {n_run} cases missed:\n" + "\n".join(missed)
