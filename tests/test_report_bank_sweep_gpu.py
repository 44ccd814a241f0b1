"""Sweep of csrc/mv_report.hip on the MI355X against the numpy restatements of tests/report_bank_cases.py.  Every output of the three
entry points is an integer, a copy or a 1.0, so the comparison is exact.  The library is called through the C ABI with buffers of
the test's own: every output sits between guard elements in a buffer pre-filled with a sentinel; after the call the elements the
contract writes hold the restatement's values and everything else -- the guards, and the plan's arrays past U / n -- still holds the
sentinel.  test_report_bank_cases_cpu.py shows that the restatements follow the rule and catch the planted defects."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from medvill_amd import hip_ops as ops        # noqa: E402
import report_bank_cases as C                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = -77777
VOCAB = 3000


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Guarded:
    """name -> a sentinel-filled flat device tensor of guard + n + guard elements; t(name) is the part the kernel is handed."""

    def __init__(self, specs, guard=C.GUARD):
        self.guard, self.n = guard, {k: n for k, (dt, n) in specs.items()}
        self.flat = {k: torch.full((n + 2 * guard,), SENTINEL if not dt.is_floating_point else -7.0, dtype=dt, device=DEV)
                     for k, (dt, n) in specs.items()}
        self.before = {k: v.clone() for k, v in self.flat.items()}

    def t(self, name):
        return self.flat[name][self.guard:self.guard + self.n[name]]

    def p(self, name):
        return self.t(name).data_ptr()

    def check(self, name, want, written=None):
        """The first `written` elements (default: all) equal `want`, bit for bit; every other element of the buffer is untouched."""
        g, n = self.guard, self.n[name]
        written = n if written is None else written
        flat, before = self.flat[name], self.before[name]
        assert torch.equal(flat[:g], before[:g]) and torch.equal(flat[g + written:], before[g + written:]), f"{name}: a guard element changed"
        got = flat[g:g + written].cpu()
        want = torch.as_tensor(want).reshape(-1)
        assert got.dtype == want.dtype and torch.equal(got, want), f"{name}: differs from the restatement"


def call(name, *args):
    ops.L.check(getattr(ops._lib(), name)(*args, ops.L.stream_ptr()), name)


def _bank_on_device(bank, dt):
    d = {k: dev(bank[k]) for k in ("txt_ids", "txt_len", "n_pred", "img_pos")}
    d["img_feats"] = dev(bank["img_feats"]).to(dt).contiguous()
    return d


def _assemble(bank_d, idx_d, fam_d, words_d, B, N, T, F, max_pred, dt, key, step, guard):
    specs = dict(input_txt=(torch.int64, B * T), segment=(torch.int64, B * T), desc=(torch.int32, 3 * B), feats=(dt, B * N * F),
                 pos=(torch.int64, B * N), masked_pos=(torch.int64, B * max_pred), masked_lm_labels=(torch.int64, B * max_pred),
                 masked_weights=(torch.float32, B * max_pred))
    out = Guarded(specs, guard)
    call("mv_report_assemble", bank_d["txt_ids"].data_ptr(), bank_d["txt_len"].data_ptr(), bank_d["n_pred"].data_ptr(),
         int(bank_d["txt_ids"].shape[0]), bank_d["img_feats"].data_ptr(), ops.L.dt_of(bank_d["img_feats"]), bank_d["img_pos"].data_ptr(),
         idx_d.data_ptr(), None if fam_d is None else fam_d.data_ptr(), B, N, T, F, max_pred, key, step,
         None if words_d is None else words_d.data_ptr(), out.p("input_txt"), out.p("segment"), out.p("desc"), out.p("feats"), out.p("pos"),
         out.p("masked_pos"), out.p("masked_lm_labels"), out.p("masked_weights"))
    torch.cuda.synchronize()
    return out


def _plan(pos_d, lab_d, w_d, vl_d, B, P, L, V):
    n = B * P
    specs = dict(rows=(torch.int32, n), row_ptr=(torch.int32, n + 1), labels=(torch.int32, n), weights=(torch.float32, n),
                 sample=(torch.int32, n), counts=(torch.int32, 4), work=(torch.int32, 3 * B))
    out = Guarded(specs)
    call("mv_report_plan", pos_d.data_ptr(), lab_d.data_ptr(), w_d.data_ptr(), None if vl_d is None else vl_d.data_ptr(), B, P, L, V,
         out.p("work"), out.p("rows"), out.p("row_ptr"), out.p("labels"), out.p("weights"), out.p("sample"), out.p("counts"))
    torch.cuda.synchronize()
    return out


def _check_plan(out, ref):
    U, n = int(ref["counts"][0]), int(ref["counts"][1])
    out.check("counts", ref["counts"])
    out.check("rows", ref["rows"], U)
    out.check("row_ptr", ref["row_ptr"], U + 1)
    for k in ("labels", "weights", "sample"):
        out.check(k, ref[k], n)


def _sweep_id(c):
    return "T{}-B{}-P{}-N{}-F{}-{}-{}".format(*c)


@pytest.mark.parametrize("case", C.SWEEP + C.COPY_CASES, ids=_sweep_id)
def test_assemble_and_plan_equal_the_restatement(case):
    T, B, max_pred, N, F, dtn, kind = case
    dt = DT[dtn]
    guard = C.GUARD_ODD if kind == "odd-guard" else C.GUARD
    seed = T * 1000 + B
    n_items = max(3, min(B, 40))
    bank = C.make_bank(n_items, T, N, F, seed, max_pred=max_pred, mask_prob=0.3, vocab=VOCAB)
    g = np.random.default_rng(seed)
    idx = g.integers(0, n_items, B).astype(np.int32)
    idx[0], idx[-1] = 0, 1                                                 # len = 1 and len = T; B > n_items repeats items anyway
    if B >= 3:
        idx[1] = idx[2]                                                    # a repeated item side by side
    family = None if kind == "hash" else g.choice([C.FAMILY_S2S, C.FAMILY_BAR, C.FAMILY_1D], B).astype(np.int32)
    key, step = 0xC0FFEE + seed, 3 + B
    words = C.draws(key, step, B, T) if kind in ("hash", "odd-guard") else C.injected_draws(B, T, seed, kind)
    injected = kind not in ("hash", "odd-guard")
    bank_d = _bank_on_device(bank, dt)
    idx_d, fam_d = dev(idx), None if family is None else dev(family)
    words_d = ops._words_to_i32(torch.from_numpy(words.astype(np.int64))).to(DEV).contiguous() if injected else None
    ref = C.assemble(bank, idx, max_pred, words, family)
    runs = [_assemble(bank_d, idx_d, fam_d, words_d, B, N, T, F, max_pred, dt, key, step, guard) for _ in range(2)]
    for out in runs:
        for k in ("input_txt", "segment", "desc", "pos", "masked_pos", "masked_lm_labels", "masked_weights"):
            out.check(k, ref[k])
        out.check("feats", torch.from_numpy(ref["feats"]).to(dt))       # the bank's values are exact in every encoding: a copy
    for k in runs[0].flat:                                                 # two runs: bitwise equal, guards included
        assert torch.equal(runs[0].flat[k].view(torch.uint8), runs[1].flat[k].view(torch.uint8)), k
    # the plan of these lists, under the valid lengths the descriptors carry
    L, out = N + T + 2, runs[0]
    vl = ref["desc"][:, 2].copy()
    pref = C.plan(ref["masked_pos"], ref["masked_lm_labels"], ref["masked_weights"], L, VOCAB, vl)
    assert pref["counts"][2] == 0 and pref["counts"][1] == int(ref["masked_weights"].sum())
    plans = [_plan(out.t("masked_pos"), out.t("masked_lm_labels"), out.t("masked_weights"), dev(vl), B, max_pred, L, VOCAB) for _ in range(2)]
    for pl in plans:
        _check_plan(pl, pref)
    for k in ("rows", "row_ptr", "labels", "weights", "sample", "counts"):
        assert torch.equal(plans[0].flat[k], plans[1].flat[k]), k


@pytest.mark.parametrize("B,T", [(1, 2), (3, 17), (64, 65), (257, 253), (5, 1024)])
def test_report_draws_equal_the_restated_hash(B, T):
    out = Guarded(dict(draws=(torch.int32, B * (T + 1))))
    call("mv_report_draws", 0xABCDEF0123456789, 11, B, T, out.p("draws"))
    torch.cuda.synchronize()
    want = C.draws(0xABCDEF0123456789, 11, B, T)
    out.check("draws", ops._words_to_i32(torch.from_numpy(want.astype(np.int64))))
    assert np.array_equal(ops.report_draws(0xABCDEF0123456789, 11, B, T, DEV).cpu().numpy().astype(np.uint64), want)


@pytest.mark.parametrize("kind", ["plain", "duplicates", "zero_weight", "label0", "fractional", "all_zero", "valid_len"])
@pytest.mark.parametrize("B,P", [(5, 6), (1, 1), (3, 64), (257, 10)])
def test_plan_cases_equal_the_restatement(kind, B, P):
    if kind == "duplicates" and P < 3:
        kind = "plain"
    L, V = 40, 300
    pos, lab, w, vl = C.plan_case(kind, B=B, P=P, L=L, V=V, seed=B * 100 + P)
    out = _plan(dev(pos), dev(lab), dev(w), None if vl is None else dev(vl), B, P, L, V)
    _check_plan(out, C.plan(pos, lab, w, L, V, vl))


@pytest.mark.parametrize("kind", C.BAD_KINDS)
def test_plan_counts_and_drops_bad_entries(kind):
    L, V = 40, 300
    pos, lab, w, vl = C.plan_case("duplicates")
    vl = C.spoil(kind, pos, lab, w, vl, L, V)
    ref = C.plan(pos, lab, w, L, V, vl)
    assert ref["counts"][2] == 1
    _check_plan(_plan(dev(pos), dev(lab), dev(w), None if vl is None else dev(vl), 5, 6, L, V), ref)


def test_plan_at_its_largest_batch():
    B, P, L, V = 2048, 64, 300, 30522
    g = np.random.default_rng(5)
    pos = g.integers(0, L + 1, (B, P)).astype(np.int64)                    # positions 0 and L occur: bad entries among them
    lab = g.integers(0, V, (B, P)).astype(np.int64)
    w = (g.integers(0, 3, (B, P)) / 2.0).astype(np.float32)
    ref = C.plan(pos, lab, w, L, V)
    assert ref["counts"][2] > 0 and ref["counts"][0] < ref["counts"][1]
    _check_plan(_plan(dev(pos), dev(lab), dev(w), None, B, P, L, V), ref)


def test_wrappers_equal_the_direct_calls():
    T, B, max_pred, N, F = 17, 5, 4, 3, 8
    bank = C.make_bank(6, T, N, F, 2, max_pred=max_pred, mask_prob=0.3, vocab=VOCAB)
    bank_d = _bank_on_device(bank, torch.float16)
    idx = np.array([0, 1, 4, 4, 2], np.int32)
    for words in (None, C.injected_draws(B, T, 1)):
        got = ops.report_assemble(bank_d["txt_ids"], bank_d["txt_len"], bank_d["n_pred"], bank_d["img_feats"], bank_d["img_pos"], dev(idx),
                                  max_pred, key=5, step=6, draws=None if words is None else torch.from_numpy(words.astype(np.int64)))
        ref = C.assemble(bank, idx, max_pred, C.draws(5, 6, B, T) if words is None else words)
        for k in ("input_txt", "segment", "desc", "pos", "masked_pos", "masked_lm_labels", "masked_weights"):
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
        assert np.array_equal(got["feats"].float().cpu().numpy(), ref["feats"])
        dp = ops.report_plan(got["masked_pos"], got["masked_lm_labels"], got["masked_weights"], N + T + 2, VOCAB)
        pref = C.plan(ref["masked_pos"], ref["masked_lm_labels"], ref["masked_weights"], N + T + 2, VOCAB)
        U, n, bad, _ = dp["counts"].tolist()
        assert [U, n, bad] == pref["counts"][:3].tolist()
        assert dp["rows"][:U].tolist() == pref["rows"].tolist() and dp["row_ptr"][:U + 1].tolist() == pref["row_ptr"].tolist()
        assert dp["labels"][:n].tolist() == pref["labels"].tolist() and dp["sample"][:n].tolist() == pref["sample"].tolist()
