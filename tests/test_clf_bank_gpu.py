"""Diagnosis-classification fine-tuning and evaluation from a device-resident bank on the MI355X: CXRBertForClassification.fit_step /
evaluate over a data.ClassificationBank against the host route -- the same model fed the batch that the numpy restatement of
tests/clf_bank_cases.py builds for the same samples.  The tiny configuration and the shapes are test_vqa_bank_gpu.py's; the gradient
measure and the tolerances are those of test_report_bank_gpu.py: LTOL on a loss (1e-4 f32, 1e-2 16-bit) and RTOL on a gradient by that
file's norm-relative measure (2e-4 f32, 3e-2 16-bit).

No loss is compared with `==`: mv_bce_multilabel adds the rows' BCE sums with f32 atomics in the order in which they finish (the header
of test_vqa_bank_gpu.py has the measured one-ulp example).  What is defined exactly is compared exactly: the logits of the two routes,
the probabilities, the integer counters and every metric that follows from them.

The file is ONE test item that walks its checks in the order below, each in f32 / bf16 / f16 where it says so (a few seconds in all,
most of it building the tiny model).  A check that misses an assertion does not end the walk; the test fails at the end with the name
and the assertion of every check that missed.  Any other error (a HIP error among them) ends it at once."""
import os
import sys
import traceback

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                     # noqa: E402
from medvill_amd import classification as K  # noqa: E402
from oracle import cxrbert_oracle as O       # noqa: E402
from oracle import synth                     # noqa: E402
import clf_bank_cases as C                   # noqa: E402
from test_report_bank_gpu import LTOL, RTOL, _cfg_dict, _compare_grads      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = O.CONFIGS["c1"]
N_REG, S_TXT, BATCH, N_IMAGES, N_SAMPLES, NC = 16, 45, 4, 6, 10, 14
T_TXT = S_TXT + 1
IDX = [8, 1, 9, 8]                           # a repeated sample
UNREACHED = ("bert.mlm.", "bert.itm.")
FAMILY_OF = {"s2s": "s2s", "bi": "1d", "bar": "bar"}
S_IMG = [0, 1, 1, 2, 5, 5, 5, 3, 4, 0]       # several samples per image
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _model(dtype, P, cfg=None, n_classes=NC, **kw):
    if dtype == torch.bfloat16:
        kw = dict(fwd_operand="bf16", grad_operand="bf16", **kw)
    m = mv.CXRBertForClassification(cfg or _cfg_dict(CFG), dtype=torch.float32 if dtype == torch.float32 else torch.bfloat16, device=DEV,
                                    n_classes=n_classes, **kw)
    if P is not None:
        m.bert.load_state_dict(P, strict=True)
    m.reset_head(seed=5)
    m.eval()
    return m


_SRC = {}


def _source():
    """The data set as numpy, in the layout of clf_bank_cases: N_SAMPLES samples over N_IMAGES images; sample 0 has no label, sample 1
    every class, every class has a positive and a negative."""
    if not _SRC:
        b = synth.make_batch(CFG, N_SAMPLES, N_REG, S_TXT, "s2s", seed=11)
        hot = np.random.default_rng(7).random((N_SAMPLES, NC)) < 0.35
        hot[0], hot[1], hot[2], hot[3] = False, True, False, True
        hot[2, ::2], hot[3, ::3] = True, False
        _SRC.update(txt_ids=b["input_txt"], txt_len=b["n_ids"].astype(np.int32), img_feats=b["img_feats"][:N_IMAGES],
                    img_pos=b["img_pos"][:N_IMAGES], s_img=np.array(S_IMG, np.int32), hot=hot, lab_bits=C.pack_bits(hot),
                    classes=[np.nonzero(h)[0].tolist() for h in hot])
    return dict(_SRC)


def _bank(m, n_classes=NC, ragged=True):
    s = _source()
    bank = mv.data.ClassificationBank(m, n_classes=n_classes)
    bank.add_images((torch.from_numpy(s["img_feats"]), torch.from_numpy(s["img_pos"])))
    labels = s["classes"] if ragged else s["hot"]
    if n_classes != NC:
        labels = [[0]] * N_SAMPLES
    bank.add_samples(torch.from_numpy(s["txt_ids"]), torch.from_numpy(s["txt_len"]), labels, image_item=s["s_img"])
    return bank


def _host_batch(bank, s, idx, mode, how="desc"):
    """What the host route feeds the model: the restatement's batch for the samples `idx`, the features in the bank's encoding."""
    B = len(idx)
    modes = [mode] * B if isinstance(mode, str) else list(mode)
    r = C.assemble(dict(s, img_feats=bank.img_feats.float().cpu().numpy()), idx, NC)
    n_ids = torch.from_numpy(s["txt_len"][idx].astype(np.int64))
    if how == "desc":
        mask = mv.data.MaskDesc.make([FAMILY_OF[m_] for m_ in modes], N_REG, S_TXT, n_ids, DEV)
    else:
        mask = mv.data.build_mask(FAMILY_OF[mode], N_REG, S_TXT, n_ids, DEV)
    args = (torch.full((B, 1), 101, dtype=torch.int64, device=DEV), torch.from_numpy(r["input_txt"]).to(DEV), mask,
            torch.from_numpy(r["segment"]).to(DEV),
            (torch.from_numpy(r["feats"]).to(DEV, bank.feat_dtype), torch.from_numpy(r["pos"]).to(DEV)),
            torch.full((B, 1), 102, dtype=torch.int64, device=DEV))
    return args, torch.from_numpy(r["target"])


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_assemble_feeds_forward(dtype):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)
    s = _source()
    bank = _bank(m, ragged=dtype != torch.float16)
    for how in ("dense", "desc"):
        for mode in ("s2s", "bi", "bar"):
            with torch.no_grad():
                out = bank.assemble(IDX, mode=mode)
                assert len(out) == 7 and isinstance(out[2], mv.data.MaskDesc) and out[2].L == T_TXT + N_REG + 2
                assert out[2].host_desc().tolist() == out[2].desc.cpu().tolist()          # the host copy is what the kernel wrote
                got = m(*out[:6])
                loss = float(m(*out[:6], labels=out[6]))
                args, target = _host_batch(bank, s, IDX, mode, how)
                want = m(*args)
                want_loss = float(m(*args, labels=target))
            assert _same_bits(got, want), (how, mode)                                      # every logit, bit for bit
            assert abs(loss - want_loss) < LTOL[dtype]
            assert torch.equal(out[6].cpu(), bank.dense_targets(IDX)) and torch.equal(out[6].cpu(), target)
    assert torch.equal(bank.assemble(IDX)[2].desc[:, 0].cpu(), torch.full((4,), 4, dtype=torch.int32))      # the default: the 1-D family


def _check_modes_per_sample_and_device_idx():
    P = O.make_params(CFG, seed=3)
    m = _model(torch.float16, P)
    s = _source()
    bank = _bank(m)
    modes = ["s2s", "bi", "bar", "s2s"]
    with torch.no_grad():
        out = bank.assemble(torch.tensor(IDX, dtype=torch.int32, device=DEV), mode=modes)
        got = m(*out[:6])
        args, target = _host_batch(bank, s, IDX, modes)
        want = m(*args)
        # past the bank on the device: clamped into it
        far = bank.assemble(torch.tensor([-5, N_SAMPLES + 3], dtype=torch.int32, device=DEV))
    assert out[2].desc[:, 0].tolist() == [1, 4, 2, 1] and _same_bits(got, want) and torch.equal(out[6].cpu(), target)
    assert torch.equal(far[6].cpu(), bank.dense_targets([0, N_SAMPLES - 1]))


def _grads(m):
    return {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}


def _check_fit_step_gradients(dtype):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)                                                   # eval mode: no dropout, the two backwards see one forward
    s = _source()
    bank = _bank(m)
    m.set_pos_weight(bank.pos_weight())
    opt = mv.optim.BertAdam(m.parameters(), lr=0.0, weight_decay=0.0)       # lr 0: the step moves nothing, the gradients stay
    m.reset_stats()
    loss = m.fit_step(bank, IDX, opt, mode="bi")
    assert loss.grad_fn is None and loss.is_cuda
    got, stats = _grads(m), m.clf_stats.cpu().clone()
    args, target = _host_batch(bank, s, IDX, "bi")
    opt.zero_grad()
    m.reset_stats()
    want_loss = m(*args, labels=target)
    want_loss.backward()
    ref = {k: g for k, g in _grads(m).items() if not k.startswith(UNREACHED)}
    assert abs(float(loss) - float(want_loss.detach())) < LTOL[dtype]
    assert torch.equal(stats, m.clf_stats.cpu()) and float(stats.sum()) > 0      # {tp, fp, fn}: integers, as after forward
    assert len(ref) > 30 and any(k.startswith("clf.") for k in ref) and any("pooler" in k for k in ref)
    _compare_grads({k: torch.as_tensor(v) for k, v in got.items()}, ref, RTOL[dtype])
    for k in got:
        if k.startswith(UNREACHED):
            assert float(got[k].abs().max()) == 0.0, k


def _check_three_fit_steps(dtype):
    P = O.make_params(CFG, seed=3)
    s = _source()
    batches = [IDX, [1, 2, 4, 8], [9, 9, 5, 6]]
    torch.manual_seed(0)
    m = _model(dtype, P)
    bank = _bank(m)
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    got = [float(m.fit_step(bank, idx, opt, mode="bi")) for idx in batches]
    torch.manual_seed(0)
    m2 = _model(dtype, P)
    m2.train()
    opt = mv.optim.BertAdam(m2.parameters(), lr=1e-3, weight_decay=0.01)
    want = []
    for idx in batches:                                                    # main.py:208-217 with host-built batches
        args, target = _host_batch(bank, s, idx, "bi")
        opt.zero_grad()
        loss = m2(*args, labels=target)
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    for a, b in zip(got, want):
        assert abs(a - b) < LTOL[dtype], (got, want)


def _host_route(m, bank, s, pos_weight=None):
    """predict and the loss of forward over every sample in batches of BATCH: -> (probs [n, C] on the host, the batch means)."""
    probs, means = [], []
    for lo in range(0, N_SAMPLES, BATCH):
        idx = list(range(lo, min(N_SAMPLES, lo + BATCH)))
        args, target = _host_batch(bank, s, idx, "bi")
        with torch.no_grad():
            probs.append(m.predict(*args).cpu())
            means.append(float(m(*args, labels=target)))
    return torch.cat(probs), means


def _check_evaluate(dtype):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)
    s = _source()
    bank = _bank(m)
    m.set_pos_weight(bank.pos_weight())
    m.train()                                                              # evaluate runs in eval mode whatever the module's mode
    eng = m.bert.engine
    state = (eng.training, eng.keep_acts, eng.drop_counter)
    out = m.evaluate(bank, batch_size=BATCH)                               # 4 + 4 + 2: a partial last batch
    assert (eng.training, eng.keep_acts, eng.drop_counter) == state and m.training
    assert set(out) == {"loss", "auroc_per_class", "macro_auroc", "micro_auroc", "macro_f1", "micro_f1", "n", "counters", "probs"}
    want_probs, means = _host_route(m.eval(), bank, s)
    m.train()
    assert out["n"] == N_SAMPLES and out["probs"].is_cuda and _same_bits(out["probs"].cpu(), want_probs)
    idx = np.arange(N_SAMPLES, dtype=np.int32)
    cnt = C.counts(out["probs"].cpu().numpy(), idx, s["lab_bits"], NC)
    assert out["counters"].dtype == torch.int64 and np.array_equal(out["counters"].numpy(), cnt)
    ref = K.metrics(out["probs"], bank.dense_targets(idx))
    for k, v in ref.items():
        assert out[k] == v, (k, out[k], v)
    assert (cnt[:NC, C.N_POS] > 0).all() and (cnt[:NC, C.N_NEG] > 0).all()      # every class has both label values here
    assert abs(out["loss"] - sum(means) / len(means)) < LTOL[dtype]
    # a subset given on the host with a per-sample mode list and a batch size past the set; the same set listed on the device
    sub = m.evaluate(bank, idx=[9, 0, 9], batch_size=64, mode=["bi", "s2s", "bar"])
    assert sub["n"] == 3 and tuple(sub["probs"].shape) == (3, NC) and int(sub["counters"][NC, :2].sum()) == 3 * NC
    on_dev = m.evaluate(bank, idx=torch.arange(N_SAMPLES, dtype=torch.int32, device=DEV), batch_size=BATCH)
    assert torch.equal(on_dev["probs"], out["probs"]) and torch.equal(on_dev["counters"], out["counters"])
    assert all(on_dev[k] == out[k] for k in ref)


def _fit(m, bank, evaluate_first):
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    out = []
    for i in range(2):
        if evaluate_first and i == 1:
            m.evaluate(bank, batch_size=BATCH)
        loss = m.fit_step(bank, IDX, opt)
        out.append((float(loss), dict(m.bert.engine.S["drop_keys"]), m.bert.engine.drop_counter))
    return out


def _check_dropout_keys_after_evaluate():
    P = O.make_params(CFG, seed=3)
    runs = []
    for ev in (False, True):
        torch.manual_seed(0)
        m = _model(torch.bfloat16, P)
        runs.append(_fit(m, _bank(m), ev))
    for (l0, k0, c0), (l1, k1, c1) in zip(*runs):
        assert k0 == k1 and c0 == c1
        assert abs(l0 - l1) < 1e-3 * abs(l0)                               # (f32 atomics: the two runs agree to rounding, not bit for bit)


def _check_refusals(monkeypatch):
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3)
    s = _source()
    empty = mv.data.ClassificationBank(m)
    with pytest.raises(ValueError, match="empty"):
        m.fit_step(empty, IDX, opt)
    empty.add_images((torch.from_numpy(s["img_feats"]), torch.from_numpy(s["img_pos"])))
    with pytest.raises(ValueError, match="empty"):
        m.evaluate(empty)
    with pytest.raises(ValueError, match="classes"):
        m.fit_step(_bank(m, n_classes=NC + 1), IDX, opt)
    with pytest.raises(ValueError, match="classes"):
        m.evaluate(_bank(m, n_classes=3))
    bank = _bank(m)
    with pytest.raises(IndexError):
        m.fit_step(bank, [0, N_SAMPLES], opt)
    with pytest.raises(IndexError):
        m.evaluate(bank, idx=[-1, 2])
    with pytest.raises(TypeError):                                          # idx on the device: int32 only
        m.fit_step(bank, torch.tensor(IDX, dtype=torch.int64, device=DEV), opt)
    with pytest.raises(TypeError):
        m.evaluate(bank, idx=torch.tensor(IDX, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="batch_size"):
        m.evaluate(bank, batch_size=0)
    with pytest.raises(ValueError, match="mode"):
        m.evaluate(bank, mode=["bi"])
    # past the pair counter's limit: refused before any batch runs, naming the host route
    many = torch.zeros((1 << 21) // NC + 1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match=r"metrics\(\)"):
        m.evaluate(bank, idx=many)
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


def _checks(monkeypatch):
    names = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
    for check in (_check_assemble_feeds_forward, _check_fit_step_gradients, _check_three_fit_steps, _check_evaluate):
        for dtype in DTYPES:
            yield f"{check.__name__[7:]} {names[dtype]}", check, (dtype,)
    yield "modes_per_sample_and_device_idx", _check_modes_per_sample_and_device_idx, ()
    yield "dropout_keys_after_evaluate", _check_dropout_keys_after_evaluate, ()
    yield "refusals", _check_refusals, (monkeypatch,)                       # last: it patches torch.distributed for the rest of the item


def test_fit_step_and_evaluate_from_the_bank_equal_the_host_route(monkeypatch):
    missed, n_run = [], 0
    for name, check, args in _checks(monkeypatch):
        n_run += 1
        try:
            check(*args)
        except AssertionError:
            missed.append(f"---- {name}\n{traceback.format_exc(limit=-2)}")
    assert n_run == 4 * len(DTYPES) + 3
    assert not missed, f"{len(missed)} of {n_run} checks missed:\n" + "\n".join(missed)
