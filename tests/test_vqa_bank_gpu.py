"""VQA fine-tuning and evaluation from a device-resident question bank on the MI355X: CXRBertForVQA.fit_step / evaluate over a
data.VqaBank against the host route -- the same model fed the batch that the numpy restatement of tests/vqa_bank_cases.py builds for
the same questions.  The tiny configuration, the shapes, the gradient measure and the tolerances are those of test_report_bank_gpu.py:
LTOL on a loss (1e-4 f32, 1e-2 16-bit) and RTOL on a gradient by that file's norm-relative measure (2e-4 f32, 3e-2 16-bit; the step's
f32 atomics rule out bitwise equality there).

Where two routes must give the SAME loss, the comparison is exact, but not `float(a) == float(b)` on the batch loss: mv_bce_fwd_bwd adds
each row's BCE sum to stats[1] with one f32 atomicAdd per row, in the order in which the rows' blocks finish, so one batch run twice
through ONE route can return two floats (measured on an MI355X, f32, dense "bi" mask, batch [8, 1, 9, 8]: 0.6937182545661926 from the
bank and 0.6937181949615479 from the host-built batch, one ulp apart, with bitwise equal logits).  So the tests compare what is defined:
the answer logits [B, A] of the two routes are equal bit for bit, each route's BCE sum (vqa_stats[1]) is one of the values that the
kernel's B additions can give -- the rows' sums (mv_bce_fwd_bwd on one row at a time: 0 + x is exact) added in f32 in every order
(`_sums_by_order`) -- and the loss is that sum over B A by the model's own device division (`_loss_is_defined`).  A batch whose orders
all give one value is compared with `==` by that very check."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                     # noqa: E402
from medvill_amd import hip_ops as ops       # noqa: E402
from oracle import cxrbert_oracle as O       # noqa: E402
from oracle import synth                     # noqa: E402
import vqa_bank_cases as C                   # noqa: E402
from test_report_bank_gpu import LTOL, RTOL, _cfg_dict, _compare_grads      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = O.CONFIGS["c1"]
N_REG, S_TXT, BATCH, N_IMAGES, N_QUESTIONS, A = 16, 45, 4, 6, 10, 458
T_TXT = S_TXT + 1
IDX = [8, 1, 9, 8]                           # a repeated question; answer types neither, open, closed, neither
UNREACHED = ("bert.mlm.", "bert.itm.", "bert.enc.pooler.")
FAMILY_OF = {"s2s": "s2s", "bi": "1d", "bar": "bar"}
Q_IMG = [0, 1, 1, 2, 5, 5, 5, 3, 4, 0]      # several questions per image


def _model(dtype, P, cfg=None, n_answers=A, **kw):
    if dtype == torch.bfloat16:
        kw = dict(fwd_operand="bf16", grad_operand="bf16", **kw)
    m = mv.CXRBertForVQA(cfg or _cfg_dict(CFG), dtype=torch.float32 if dtype == torch.float32 else torch.bfloat16, device=DEV,
                         n_answers=n_answers, **kw)
    if P is not None:
        m.bert.load_state_dict(P, strict=True)
    m.reset_head(seed=5)
    m.eval()
    return m


_SRC = {}


def _source(answers=None):
    """The data set as numpy: N_QUESTIONS questions (tokens + [SEP] + [PAD]..., lengths counting the [SEP]) over N_IMAGES images, in
    the layout of vqa_bank_cases.  `answers` = (labels, scores) per question replaces the default sparse answers."""
    if not _SRC:
        b = synth.make_batch(CFG, N_QUESTIONS, N_REG, S_TXT, "s2s", seed=11)
        labels = [[(7 * q) % A, (11 * q + 3) % A][:q % 3] for q in range(N_QUESTIONS)]      # 0, 1 or 2 answers
        labels[9] = [A - 1, 5, A - 1]                                                       # a duplicated label: the later score wins
        scores = [[1.0, 0.6, 0.3][:len(l)] for l in labels]
        _SRC.update(txt_ids=b["input_txt"], txt_len=b["n_ids"].astype(np.int32), img_feats=b["img_feats"][:N_IMAGES],
                    img_pos=b["img_pos"][:N_IMAGES], q_img=np.array(Q_IMG, np.int32), ans_type=(np.arange(N_QUESTIONS) % 3).astype(np.int32),
                    group=np.array([0, 1, 2, 0, 1, 2, 0, 1, 7, 7], np.int32), labels=labels, scores=scores)
    s = dict(_SRC)
    if answers is not None:
        s["labels"], s["scores"] = answers
    s["ans_ptr"] = np.concatenate([[0], np.cumsum([len(l) for l in s["labels"]])]).astype(np.int32)
    s["ans_label"] = np.array([x for l in s["labels"] for x in l], np.int32)
    s["ans_score"] = np.array([x for l in s["scores"] for x in l], np.float32)
    return s


def _bank(m, s=None, n_answers=A):
    s = s or _source()
    bank = mv.data.VqaBank(m, n_answers=n_answers)
    bank.add_images((torch.from_numpy(s["img_feats"]), torch.from_numpy(s["img_pos"])))
    types = ["CLOSED", "OPEN ", "other"]
    bank.add_questions(torch.from_numpy(s["txt_ids"]), torch.from_numpy(s["txt_len"]), s["q_img"], s["labels"], s["scores"],
                       [types[t] for t in s["ans_type"]], group=s["group"])
    return bank


def _host_batch(bank, s, idx, mode, how):
    """What the host route feeds the model: the restatement's batch for the questions `idx`, the features in the bank's encoding."""
    B = len(idx)
    modes = [mode] * B if isinstance(mode, str) else list(mode)
    r = C.assemble(dict(s, img_feats=bank.img_feats.float().cpu().numpy()), idx, A)
    n_ids = torch.from_numpy(s["txt_len"][idx].astype(np.int64))
    if how == "desc":
        mask = mv.data.MaskDesc.make([FAMILY_OF[m_] for m_ in modes], N_REG, S_TXT, n_ids, DEV)
    else:
        assert isinstance(mode, str)
        mask = mv.data.build_mask(FAMILY_OF[mode], N_REG, S_TXT, n_ids, DEV)
    args = (torch.full((B, 1), 101, dtype=torch.int64, device=DEV), torch.from_numpy(r["input_txt"]).to(DEV), mask,
            torch.from_numpy(r["segment"]).to(DEV),
            (torch.from_numpy(r["feats"]).to(DEV, bank.feat_dtype), torch.from_numpy(r["pos"]).to(DEV)),
            torch.full((B, 1), 102, dtype=torch.int64, device=DEV))
    return args, dict(ans_labels=torch.from_numpy(r["target"]), ans_type=torch.from_numpy(r["ans_type"]))


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _logits(m):
    """The answer logits [B, A] of the model's last training-vector forward (the classifier's output buffer)."""
    return m._acts["logits"][:, :m.n_answers].clone()


def _sums_by_order(logits, target):
    """Every BCE sum the loss node can leave in vqa_stats[1] for these logits and targets: the rows' sums, each from mv_bce_fwd_bwd on
    that row alone, added in f32 in each of the B! orders the kernel's atomics can take."""
    B, n_ans = int(logits.shape[0]), int(target.shape[1])
    rows = []
    for i in range(B):
        st = torch.zeros(6, dtype=torch.float32, device=DEV)
        ops.bce_fwd_bwd(logits[i:i + 1], n_ans, R=1, target=target[i:i + 1].to(DEV).contiguous(), stats=st)
        rows.append(np.float32(float(st[1])))
    out = set()
    for order in itertools.permutations(range(B)):
        acc = np.float32(0.0)
        for i in order:
            acc = np.float32(acc + rows[i])
        out.add(float(acc))
    return out


def _snap(m, loss):
    """What the model's last loss forward left behind, taken before the next one replaces it."""
    st, B = m.vqa_stats, int(m.vqa_pred.numel())
    return dict(loss=float(loss), bce_sum=float(st[1]), sum_over_ba=float(st[1] / float(B * m.n_answers)), logits=_logits(m),
                stats=st.cpu(), pred=m.vqa_pred.cpu())


def _loss_is_defined(snap, allowed):
    """The BCE sum is one of `allowed`, and the loss is that sum over B A (the division the loss node does, on the device)."""
    return snap["bce_sum"] in allowed and snap["loss"] == snap["sum_over_ba"] and math.isfinite(snap["loss"])


def _same_forward(a, b, allowed):
    return _same_bits(a["logits"], b["logits"]) and _loss_is_defined(a, allowed) and _loss_is_defined(b, allowed) \
        and torch.equal(a["stats"][DEFINED_STATS], b["stats"][DEFINED_STATS]) and torch.equal(a["pred"], b["pred"])


# of vqa_stats, [2] / [4] sum the closed / open scores and [3] / [5] count them: in IDX's batch either split holds one sample, so these
# have one value in any order.  [0] and [1] are f32 atomic sums over the four rows: [1] is `_sums_by_order`'s, and [0] adds the rows'
# scores target[i, pred[i]], whose terms (pred, target) are compared exactly
DEFINED_STATS = [2, 3, 4, 5]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_assemble_feeds_forward(dtype):
    """The grid f32 / bf16 / f16 x dense mask / descriptors x "s2s" / "bi" / "bar"; the masks and modes run inside one test per dtype
    (the suite's reports stay few)."""
    for how in ("dense", "desc"):
        for mode in ("s2s", "bi", "bar"):
            _check_assemble_feeds_forward(dtype, how, mode)


def _check_assemble_feeds_forward(dtype, how, mode):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)
    s = _source()
    bank = _bank(m)
    with torch.no_grad():
        out = bank.assemble(IDX, mode=mode)
        assert len(out) == 8 and isinstance(out[2], mv.data.MaskDesc) and out[2].L == T_TXT + N_REG + 2
        assert out[2].host_desc().tolist() == out[2].desc.cpu().tolist()              # the host copy is what the kernel wrote
        got = _snap(m, m(*out[:6], ans_labels=out[6], ans_type=out[7])[1])
        args, kw = _host_batch(bank, s, IDX, mode, how)
        want = _snap(m, m(*args, **kw)[1])
        allowed = _sums_by_order(got["logits"], out[6])
    assert _same_forward(got, want, allowed)                # every answer logit bit for bit, the loss, the split statistics, the argmax
    assert torch.equal(out[6].cpu(), bank.dense_targets(IDX)) and float(got["stats"][3]) == 1.0 and float(got["stats"][5]) == 1.0


def test_modes_per_sample_and_device_idx():
    P = O.make_params(CFG, seed=3)
    m = _model(torch.float16, P)
    s = _source()
    bank = _bank(m)
    modes = ["s2s", "bi", "bar", "s2s"]
    with torch.no_grad():
        out = bank.assemble(torch.tensor(IDX, dtype=torch.int32, device=DEV), mode=modes)
        got = _snap(m, m(*out[:6], ans_labels=out[6], ans_type=out[7])[1])
        args, kw = _host_batch(bank, s, IDX, modes, "desc")
        want = _snap(m, m(*args, **kw)[1])
        allowed = _sums_by_order(got["logits"], out[6])
    assert out[2].desc[:, 0].tolist() == [1, 4, 2, 1] and _same_forward(got, want, allowed)


def _grads(m):
    return {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_fit_step_gradients():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        _check_fit_step_gradients(dtype)


def _check_fit_step_gradients(dtype):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)                                                   # eval mode: no dropout, the two backwards see one forward
    s = _source()
    bank = _bank(m)
    opt = mv.optim.BertAdam(m.parameters(), lr=0.0, weight_decay=0.0)       # lr 0: the step moves nothing, the gradients stay
    loss = m.fit_step(bank, IDX, opt, mode="bi")
    assert loss.grad_fn is None and m.vqa_pred is not None
    got, mine = _grads(m), _snap(m, loss)
    args, kw = _host_batch(bank, s, IDX, "bi", "desc")
    opt.zero_grad()
    _, want_loss = m(*args, **kw)
    want_loss.backward()
    theirs = _snap(m, want_loss.detach())
    ref = {k: g for k, g in _grads(m).items() if not k.startswith(UNREACHED)}
    assert _same_forward(mine, theirs, _sums_by_order(mine["logits"], bank.dense_targets(IDX)))
    assert len(ref) > 30 and any(k.startswith("ans_classifier.") for k in ref)
    _compare_grads({k: torch.as_tensor(v) for k, v in got.items()}, ref, RTOL[dtype])
    for k in got:
        if k.startswith(UNREACHED):
            assert float(got[k].abs().max()) == 0.0, k


def test_three_fit_steps():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        _check_three_fit_steps(dtype)


def _check_three_fit_steps(dtype):
    P = O.make_params(CFG, seed=3)
    s = _source()
    batches = [IDX, [1, 2, 4, 8], [9, 9, 5, 6]]
    torch.manual_seed(0)
    m = _model(dtype, P)
    bank = _bank(m)
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    got, first = [], None
    for idx in batches:
        loss = m.fit_step(bank, idx, opt, mode="bi")
        got.append(float(loss))
        first = _snap(m, loss) if first is None else first
    torch.manual_seed(0)
    m2 = _model(dtype, P)
    m2.train()
    opt = mv.optim.BertAdam(m2.parameters(), lr=1e-3, weight_decay=0.01)
    want = []
    for idx in batches:                                                    # finetune.py:443-451 with host-built batches
        args, kw = _host_batch(bank, s, idx, "bi", "desc")
        opt.zero_grad()
        _, loss = m2(*args, **kw)
        loss.backward()
        opt.step()
        if not want:                                                       # the first step: the same launches on the same parameters
            assert _same_forward(first, _snap(m2, loss.detach()), _sums_by_order(first["logits"], bank.dense_targets(idx)))
        want.append(float(loss.detach()))
    for a, b in zip(got, want):
        assert abs(a - b) < LTOL[dtype], (got, want)


def _host_predictions(m, bank, s, path, mode="bi"):
    """The host route over every question in batches of BATCH: -> (pred [n] on the host, BCE sum)."""
    preds, bce = [], 0.0
    for lo in range(0, N_QUESTIONS, BATCH):
        idx = list(range(lo, min(N_QUESTIONS, lo + BATCH)))
        args, kw = _host_batch(bank, s, idx, mode, "desc")
        with torch.no_grad():
            if path == "inference":
                preds.append(m.predict(*args).cpu())
            else:
                m(*args, **kw)
                preds.append(m.vqa_pred.cpu())
                bce += float(m.vqa_stats[1])
    return torch.cat(preds), bce


def test_evaluate():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for path in ("inference", "train"):
            _check_evaluate(dtype, path)


def _check_evaluate(dtype, path):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)
    m.train()                                                              # evaluate runs in eval mode whatever the module's mode
    first = _host_predictions(m.eval(), _bank(m), _source(), path)[0].tolist()
    m.train()
    # answers that make the score worth checking: questions 0, 3, 6, 9 list their own prediction (9 twice: the later score), 1, 4, 7
    # list it second, the others list another column or nothing
    labels = [[p] if q % 3 == 0 else ([(p + 1) % A, p] if q % 3 == 1 else [(p + 2) % A][:q % 2]) for q, p in enumerate(first)]
    labels[9] = [first[9], 5, first[9]]
    scores = [[1.0, 0.6, 0.3][:len(l)] for l in labels]
    s = _source((labels, scores))
    bank = _bank(m, s)
    eng = m.bert.engine
    state = (eng.training, eng.keep_acts, eng.drop_counter)
    out = m.evaluate(bank, batch_size=BATCH, path=path)
    assert (eng.training, eng.keep_acts, eng.drop_counter) == state and m.training
    want_pred, bce = _host_predictions(m.eval(), bank, s, path)
    assert out["pred"].dtype == torch.int64 and torch.equal(out["pred"].cpu(), want_pred) and want_pred.tolist() == first
    idx = np.arange(N_QUESTIONS, dtype=np.int32)
    sc, cnt = C.score(s, want_pred.numpy(), idx, 8)
    assert out["score"].cpu().numpy().tobytes() == sc.tobytes()
    ref = C.metrics(cnt)
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
    for k in ("acc", "closed_acc", "open_acc", "n", "closed_n", "open_n"):
        assert same(out[k], ref[k]), (k, out[k], ref[k])
    assert set(out["by_group"]) == set(ref["by_group"]) == {0, 1, 2, 7}
    for g, r in ref["by_group"].items():
        assert all(same(out["by_group"][g][k], r[k]) for k in r), g
    # closed: questions 0, 3, 6 score 1.0 and question 9 the later 0.3; open: questions 1, 4, 7 score 0.6; the others score nothing
    f = lambda v: float(np.float32(v))
    assert out["n"] == 10 and out["closed_n"] == 4 and out["open_n"] == 3
    assert out["closed_acc"] == (3.0 + f(0.3)) / 4 and out["open_acc"] == f(0.6) and abs(out["acc"] - 0.51) < 1e-6
    assert math.isnan(out["by_group"][7]["open_acc"]) and out["by_group"][7]["closed_acc"] == f(0.3)     # questions 8 (neither), 9 (closed)
    assert math.isnan(out["by_group"][2]["closed_acc"]) and out["by_group"][2]["acc"] == 0.0 and out["by_group"][2]["n"] == 2
    if path == "train":
        assert abs(out["loss"] - bce / (N_QUESTIONS * A)) < LTOL[dtype]
    else:
        assert "loss" not in out
    # a subset given on the host, a per-question mode list and a batch size past the set
    sub = m.evaluate(bank, idx=[9, 0, 9], batch_size=64, path=path, mode=["bi", "s2s", "bar"])
    assert sub["n"] == 3 and sub["pred"].numel() == 3 and sub["score"][0] == sub["score"][2]
    # the same set listed on the device
    on_dev = m.evaluate(bank, idx=torch.arange(N_QUESTIONS, dtype=torch.int32, device=DEV), batch_size=BATCH, path=path)
    assert torch.equal(on_dev["pred"], out["pred"]) and on_dev["acc"] == out["acc"] and on_dev["by_group"].keys() == out["by_group"].keys()


def _fit(m, bank, evaluate_first):
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    out = []
    for i in range(2):
        if evaluate_first and i == 1:
            m.evaluate(bank, batch_size=BATCH, path="train")
            m.evaluate(bank, batch_size=BATCH)
        loss = m.fit_step(bank, IDX, opt)
        out.append((float(loss), dict(m.bert.engine.S["drop_keys"]), m.bert.engine.drop_counter))
    return out


def test_dropout_keys_after_evaluate():
    P = O.make_params(CFG, seed=3)
    runs = []
    for ev in (False, True):
        torch.manual_seed(0)
        m = _model(torch.bfloat16, P)
        runs.append(_fit(m, _bank(m), ev))
    for (l0, k0, c0), (l1, k1, c1) in zip(*runs):
        assert k0 == k1 and c0 == c1
        assert abs(l0 - l1) < 1e-3 * abs(l0)                               # (f32 atomics: the two runs agree to rounding, not bit for bit)


def test_refusals(monkeypatch):
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3)
    s = _source()
    empty = mv.data.VqaBank(m)
    with pytest.raises(ValueError, match="empty"):
        m.fit_step(empty, IDX, opt)
    empty.add_images((torch.from_numpy(s["img_feats"]), torch.from_numpy(s["img_pos"])))
    with pytest.raises(ValueError, match="empty"):
        m.evaluate(empty)
    with pytest.raises(ValueError, match="answers"):
        m.fit_step(_bank(m, n_answers=A + 1), IDX, opt)
    with pytest.raises(ValueError, match="answers"):
        m.evaluate(_bank(m, _source(([[0]] * N_QUESTIONS, [[1.0]] * N_QUESTIONS)), n_answers=17))
    bank = _bank(m)
    with pytest.raises(IndexError):
        m.fit_step(bank, [0, N_QUESTIONS], opt)
    with pytest.raises(IndexError):
        m.evaluate(bank, idx=[-1, 2])
    with pytest.raises(TypeError):                                          # idx on the device: int32 only
        m.fit_step(bank, torch.tensor(IDX, dtype=torch.int64, device=DEV), opt)
    with pytest.raises(TypeError):
        m.evaluate(bank, idx=torch.tensor(IDX, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="path"):
        m.evaluate(bank, path="both")
    short = _model(torch.bfloat16, None, cfg=_cfg_dict(CFG, max_position_embeddings=N_REG + T_TXT + 1))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        short.evaluate(_bank(short))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        short.fit_step(_bank(short), IDX, mv.optim.BertAdam(short.parameters(), lr=1e-3))
    # several ranks: a gradient step is refused before anything runs
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="data-parallel"):
        m.fit_step(bank, IDX, opt)
