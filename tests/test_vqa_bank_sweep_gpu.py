"""Sweep of csrc/mv_vqa_bank.hip on the MI355X against the numpy restatements of tests/vqa_bank_cases.py.  Every output of the two entry
points is an integer, a copied bit pattern or an f32 taken from the bank, so the comparison is exact (target and score as f32 bit
patterns, the counters as integers after two accumulating launches into one block).  The library is called through the C ABI with
buffers of the test's own: every output sits between guard elements in a buffer pre-filled with a sentinel; after the call the elements
the contract writes hold the restatement's values and the guards still hold the sentinel.  test_vqa_bank_cases_cpu.py shows that the
case set reaches every branch of the launcher and that this comparison catches the planted defects."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from medvill_amd import hip_ops as ops        # noqa: E402
import vqa_bank_cases as C                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = -77777


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Guarded:
    """name -> a sentinel-filled flat device tensor of guard + n + guard elements; t(name) is the part the kernel is handed."""

    def __init__(self, specs, guard=C.GUARD):
        self.guard, self.n = guard, {k: n for k, (dt, n) in specs.items()}
        self.flat = {k: torch.full((n + 2 * guard,), SENTINEL if not dt.is_floating_point else -7.0, dtype=dt, device=DEV)
                     for k, (dt, n) in specs.items()}
        self.before = {k: (v[:guard].clone(), v[guard + self.n[k]:].clone()) for k, v in self.flat.items()}

    def t(self, name):
        return self.flat[name][self.guard:self.guard + self.n[name]]

    def p(self, name):
        return self.t(name).data_ptr()

    def check(self, name, want):
        """The written elements equal `want`, bit for bit; the guard elements on both sides are untouched."""
        g, n = self.guard, self.n[name]
        flat, (lo, hi) = self.flat[name], self.before[name]
        assert torch.equal(flat[:g], lo) and torch.equal(flat[g + n:], hi), f"{name}: a guard element changed"
        got, want = flat[g:g + n].cpu(), torch.as_tensor(want).reshape(-1)
        assert got.dtype == want.dtype and got.shape == want.shape, name
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        assert torch.equal(got.view(bits), want.view(bits)), f"{name}: differs from the restatement"


def call(name, *args):
    ops.L.check(getattr(ops._lib(), name)(*args, ops.L.stream_ptr()), name)


def _bank_on_device(bank, dt):
    d = {k: dev(bank[k]) for k in ("txt_ids", "txt_len", "q_img", "ans_ptr", "ans_label", "ans_score", "ans_type", "group", "img_pos")}
    d["img_feats"] = dev(bank["img_feats"]).to(dt).contiguous()
    return d


def _assemble(bd, idx_d, fam_d, B, N, T, F, A, dt, guard):
    specs = dict(input_txt=(torch.int64, B * T), segment=(torch.int64, B * T), desc=(torch.int32, 3 * B), feats=(dt, B * N * F),
                 pos=(torch.int64, B * N), target=(torch.float32, B * A), ans_type=(torch.int32, B))
    out = Guarded(specs, guard)
    call("mv_vqa_assemble", bd["txt_ids"].data_ptr(), bd["txt_len"].data_ptr(), bd["q_img"].data_ptr(), int(bd["txt_ids"].shape[0]),
         bd["ans_ptr"].data_ptr(), bd["ans_label"].data_ptr(), bd["ans_score"].data_ptr(), int(bd["ans_label"].numel()),
         bd["ans_type"].data_ptr(), bd["img_feats"].data_ptr(), ops.L.dt_of(bd["img_feats"]), bd["img_pos"].data_ptr(),
         int(bd["img_feats"].shape[0]), idx_d.data_ptr(), None if fam_d is None else fam_d.data_ptr(), B, N, T, F, A, out.p("input_txt"),
         out.p("segment"), out.p("desc"), out.p("feats"), out.p("pos"), out.p("target"), out.p("ans_type"))
    torch.cuda.synchronize()
    return out


def _score(bd, pred_d, idx_d, use_group, G, out):
    call("mv_vqa_score", pred_d.data_ptr(), idx_d.data_ptr(), int(pred_d.numel()), int(bd["txt_ids"].shape[0]), bd["ans_ptr"].data_ptr(),
         bd["ans_label"].data_ptr(), bd["ans_score"].data_ptr(), int(bd["ans_label"].numel()), bd["ans_type"].data_ptr(),
         bd["group"].data_ptr() if use_group else None, G, out.p("score"), out.p("counters"))
    torch.cuda.synchronize()


def _sweep_id(c):
    return "B{}-A{}-T{}-NF{}-{}{}".format(c[0], c[1], c[2], c[3] * c[4], c[5], "-odd" if c[8] == C.GUARD_ODD else "")


@pytest.mark.parametrize("case", C.SWEEP, ids=_sweep_id)
def test_kernels_equal_the_restatement(case):
    B, A, T, N, F, dtn, fam, grp, guard = case
    dt = DT[dtn]
    bank = C.sweep_bank(case)
    idx = C.batch_idx(bank, B, seed=B + T)
    g = np.random.default_rng(B + A)
    family = None if fam is None else g.choice([C.FAMILY_S2S, C.FAMILY_BAR, C.FAMILY_1D], B).astype(np.int32)
    bd = _bank_on_device(bank, dt)
    idx_d, fam_d = dev(idx), None if family is None else dev(family)
    ref = C.assemble(bank, idx, A, family)
    large = N * F > 1 << 20
    runs = [_assemble(bd, idx_d, fam_d, B, N, T, F, A, dt, guard) for _ in range(1 if large else 2)]
    for out in runs:
        for k in ("input_txt", "segment", "desc", "pos", "target", "ans_type"):
            out.check(k, ref[k])
        out.check("feats", torch.from_numpy(ref["feats"]).to(dt))       # the bank's values are exact in every encoding: a copy
    for k in runs[0].flat:                                                 # two runs: bitwise equal, guards included
        assert torch.equal(runs[0].flat[k].view(torch.uint8), runs[-1].flat[k].view(torch.uint8)), k
    # the scores of a batch of predictions, and the counters after two accumulating launches into one block
    G = grp or 1
    pred = C.batch_pred(bank, idx, A, seed=A)
    other = np.roll(pred, 1)
    out = Guarded(dict(score=(torch.float32, B), counters=(torch.int64, G * 6)))
    out.t("counters").zero_()
    s1, c1 = C.score(bank, pred, idx, G, use_group=grp is not None)
    _score(bd, dev(pred), idx_d, grp is not None, G, out)
    out.check("score", s1)
    out.check("counters", c1)
    s2, c2 = C.score(bank, other, idx, G, use_group=grp is not None, counters=c1)
    _score(bd, dev(other), idx_d, grp is not None, G, out)
    out.check("score", s2)
    out.check("counters", c2)
    assert int(c2[:, :, 1].sum()) == 2 * B
    if grp:
        assert (c2[5] == 0).all()                                          # the empty group stays empty


def test_score_output_is_optional_and_groups_clamp():
    case = C.SWEEP[2]
    B, A = case[:2]
    bank = C.sweep_bank(case)
    idx = C.batch_idx(bank, B, seed=1)
    pred = C.batch_pred(bank, idx, A, seed=2)
    bd = _bank_on_device(bank, torch.float32)
    G = 3                                                                  # groups 3 .. 7 of the bank fall into group 2
    out = Guarded(dict(counters=(torch.int64, G * 6)))
    out.t("counters").zero_()
    pred_d, idx_d = dev(pred), dev(idx)
    call("mv_vqa_score", pred_d.data_ptr(), idx_d.data_ptr(), B, int(bd["txt_ids"].shape[0]), bd["ans_ptr"].data_ptr(),
         bd["ans_label"].data_ptr(), bd["ans_score"].data_ptr(), int(bd["ans_label"].numel()), bd["ans_type"].data_ptr(),
         bd["group"].data_ptr(), G, None, out.p("counters"))
    torch.cuda.synchronize()
    out.check("counters", C.score(bank, pred, idx, G)[1])


def test_a_bank_without_any_answer():
    B, A, T, N, F = 3, 17, 6, 2, 8
    bank = C.make_bank(6, 3, T, N, F, A, seed=4)
    bank["ans_ptr"][:] = 0
    bank["ans_label"], bank["ans_score"] = np.zeros(0, np.int32), np.zeros(0, np.float32)
    bd = _bank_on_device(bank, torch.float16)
    idx = np.array([1, 2, 5], np.int32)
    out = _assemble(bd, dev(idx), None, B, N, T, F, A, torch.float16, C.GUARD)
    ref = C.assemble(bank, idx, A)
    assert not ref["target"].any()
    for k in ("input_txt", "segment", "desc", "pos", "target", "ans_type"):
        out.check(k, ref[k])


def test_wrappers_equal_the_direct_calls():
    case = C.SWEEP[1]
    B, A, T, N, F = case[:5]
    bank = C.sweep_bank(case)
    bd = _bank_on_device(bank, torch.float16)
    idx = C.batch_idx(bank, B, seed=3)
    fam = np.array([1, 2, 4], np.int32)
    got = ops.vqa_assemble(bd["txt_ids"], bd["txt_len"], bd["q_img"], bd["ans_ptr"], bd["ans_label"], bd["ans_score"], bd["ans_type"],
                           bd["img_feats"], bd["img_pos"], dev(idx), A, family=dev(fam))
    ref = C.assemble(bank, idx, A, fam)
    for k in ("input_txt", "segment", "desc", "pos", "target", "ans_type"):
        assert got[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    assert np.array_equal(got["feats"].float().cpu().numpy(), ref["feats"])
    pred = C.batch_pred(bank, idx, A, seed=5)
    score, counters = ops.vqa_score(dev(pred), dev(idx), bd["ans_ptr"], bd["ans_label"], bd["ans_score"], bd["ans_type"], group=bd["group"])
    _, counters = ops.vqa_score(dev(pred), dev(idx), bd["ans_ptr"], bd["ans_label"], bd["ans_score"], bd["ans_type"], group=bd["group"],
                                counters=counters, want_score=False)
    s, c = C.score(bank, pred, idx, 8)
    assert score.cpu().numpy().tobytes() == s.tobytes() and tuple(counters.shape) == (8, 3, 2)
    assert np.array_equal(counters.cpu().numpy(), 2 * c)
