"""Multi-label classification fine-tuning on the MI355X: mv_bce_multilabel against torch, and CXRBertForClassification against the
oracle encoder (oracle/cxrbert_oracle.py, CPU autograd) + a torch pooler / Linear + BCEWithLogitsLoss(pos_weight) -- the reference's
MultimodalBertClf arithmetic on CXRBERT.  Patterned on tests/test_vqa_gpu.py, with its tolerances (same encoder path and precision)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import medvill_amd as mv
from medvill_amd import _lib
from medvill_amd import hip_ops as ops
from medvill_amd.classification import metrics
from oracle import cxrbert_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 14
CFG = O.CONFIGS["c1"]
FAMILIES = ["full", "s2s", "bar", "1d"]
NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("weighted", [False, True])
def test_bce_multilabel_matches_torch(gdt, weighted):
    g = torch.Generator().manual_seed(5)
    R, ld = 37, 16
    z = torch.randn(R, ld, generator=g) * 3
    z[0, :7], z[0, 7:C] = 80.0, -80.0                                  # saturated logits: finite loss, exact gradients
    y = (torch.rand(R, C, generator=g) < 0.3).float()
    w = (torch.rand(C, generator=g) * 5 + 0.2) if weighted else None
    zd, yd = z.to(DEV), y.to(DEV)
    loss = torch.zeros(1, device=DEV)
    d = torch.full((R, ld), 7.0, device=DEV).to(gdt)
    probs = torch.empty(R, C, device=DEV)
    cnt = torch.zeros(3, C, device=DEV)
    S = torch.tensor([4.0], device=DEV)
    for _ in range(2):                                                  # counters and the loss sum accumulate across calls
        ops.bce_multilabel(zd, C, ld=ld, target=yd, pos_weight=None if w is None else w.to(DEV), loss=loss, dgrad=d, ldd=ld,
                           grad_scale=0.5, loss_scale_dev=S, probs=probs, counters=cnt)
    zz = z[:, :C].double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(zz, y.double(), pos_weight=None if w is None else w.double(), reduction="sum")
    ref.backward()
    ref = float(ref.detach())
    assert torch.isfinite(loss).all() and abs(float(loss) / 2 - ref) < 1e-5 * ref
    tol = 1e-6 if gdt == torch.float32 else (2e-2 if gdt == torch.bfloat16 else 3e-3)       # test_vqa_gpu's gradient tolerances
    scale = 1.0 if w is None else float(w.max())
    assert float((d[:, :C].double().cpu() - zz.grad * 2.0).abs().max()) < tol * 2.0 * scale
    assert float(d[:, C:].float().abs().max()) == 0.0                  # padded leading dimension: padding columns written as zero
    assert float((probs.cpu() - torch.sigmoid(z[:, :C])).abs().max()) < 1e-6
    pred, pos = z[:, :C] > 0, y > 0.5
    want = torch.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)]).float() * 2
    assert torch.equal(cnt.cpu(), want)
    p2 = torch.empty(R, C, device=DEV)
    ops.bce_multilabel(zd, C, ld=ld, probs=p2)                          # inference form: probabilities only
    assert torch.equal(p2, probs)


def test_bce_multilabel_rejects_bad_arguments():
    lib = _lib.load()
    z, out = torch.zeros(4, 16, device=DEV), torch.zeros(1, device=DEV)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = _lib.stream_ptr()
    bce = lambda logits=z, R=4, C_=14, ld=16, tgt=z, loss=out, dg=None, dt=0, ldd=0: lib.mv_bce_multilabel(
        P(logits), ld, P(tgt), None, R, C_, P(loss), P(dg), dt, ldd, None, 1.0, None, None, None, st)
    assert bce(logits=None) == -1 and bce(C_=0) == -1 and bce(R=0) == -1 and bce(ld=8) == -1 and bce(tgt=None) == -1
    assert bce(dg=z, ldd=8) == -2 and bce(dg=z, ldd=16, dt=9) == -3
    torch.cuda.synchronize()
    assert float(out) == 0.0


# ------------------------------------------------------------------------------------------------ model against the oracle
def _cfg_dict(c):
    return dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)


def _labels(B, seed):
    return (torch.rand(B, C, generator=torch.Generator().manual_seed(seed)) < 0.3).float()


POS_W = torch.linspace(0.5, 4.0, C)


def _batch(family, B=4, N=16, S=45, seed=11):
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, B, N, S, family, seed=seed).items()}
    b["labels"] = _labels(B, seed)
    return b


def _model(dtype, P, seed=5, pos_weight=POS_W, cfg=CFG):
    m = mv.CXRBertForClassification(_cfg_dict(cfg), dtype=dtype, device=DEV, n_classes=C, pos_weight=pos_weight)
    m.bert.load_state_dict(P, strict=True)
    m.reset_head(seed=seed)
    m.eval()
    return m


def _inputs(b, mask=None):
    return (b["cls_tok"].to(DEV), b["input_txt"].to(DEV), b["attn_mask"].to(DEV) if mask is None else mask, b["segment"].to(DEV),
            (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))


def _reference(P, head, b, pos_weight=POS_W):
    """oracle encoder (CPU, f32 autograd) + torch pooler + Linear + BCEWithLogitsLoss(pos_weight) -> loss, grads, logits."""
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    hg = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in head.items()}
    x, _ = O.encode(Pg, CFG, b["cls_tok"], b["input_txt"], b["attn_mask"], b["segment"], b["img_feats"], b["img_pos"], b["sep_tok"])
    pooled = torch.tanh(F.linear(x[:, 0], Pg["enc.pooler.dense.weight"], Pg["enc.pooler.dense.bias"]))
    logits = F.linear(pooled, hg["clf.weight"], hg["clf.bias"])
    loss = F.binary_cross_entropy_with_logits(logits, b["labels"], pos_weight=pos_weight)
    loss.backward()
    grads = {k: p.grad for k, p in Pg.items() if p.grad is not None}
    grads.update({k: p.grad for k, p in hg.items()})
    return float(loss.detach()), grads, logits.detach()


def _head(m):
    return {k: p.detach() for k, p in m.clf.named_parameters(prefix="clf")}


def _grads(m):
    out = {k: p.grad for k, p in m.bert.named_parameters()}
    out.update({k: p.grad for k, p in m.clf.named_parameters(prefix="clf")})
    return out


def _compare_grads(got, ref, rtol):          # as tests/test_vqa_gpu.py compares them
    gmax = max(float(g.abs().max()) for g in ref.values())
    floor = (1e-5 if rtol < 1e-3 else 3e-2) * gmax
    for k, r in ref.items():
        g = got[k].float().cpu()
        n = r.double().norm()
        e1 = float((g.double() - r.double()).norm()) / max(float(n), floor * r.numel() ** 0.5)
        assert e1 < rtol, (k, e1, float(n))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype,ltol,rtol", [(torch.float32, 1e-4, 2e-4), (torch.bfloat16, 1e-2, 3e-2)])
def test_loss_and_every_gradient_match_the_oracle(family, dtype, ltol, rtol):
    P = O.make_params(CFG, seed=3)
    b = _batch(family)
    m = _model(dtype, P)
    loss = m(*_inputs(b), labels=b["labels"].to(DEV))
    loss.backward()
    ref_loss, ref_g, ref_logits = _reference(P, _head(m), b)
    print(f"clf {family} {dtype}: loss {float(loss.detach()):.6f} oracle {ref_loss:.6f}")
    assert abs(float(loss.detach()) - ref_loss) < ltol, (float(loss.detach()), ref_loss)
    _compare_grads(_grads(m), ref_g, rtol)
    g = dict(m.bert.named_parameters())
    assert float(g["enc.pooler.dense.weight"].grad.abs().max()) > 0 and float(ref_g["enc.pooler.dense.weight"].abs().max()) > 0
    for k, p in g.items():                       # the ITM and MLM heads get no gradient (the model has neither)
        if k.startswith(("itm.", "mlm.")):
            assert float(p.grad.abs().max()) == 0.0, k
    pred, pos = ref_logits > 0, b["labels"] > 0.5
    if dtype == torch.float32 and float(ref_logits.abs().min()) > 1e-4:
        want = torch.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)]).float()
        assert torch.equal(m.clf_stats.cpu(), want)
    probs = m.predict(*_inputs(b)).cpu()
    assert float((probs - torch.sigmoid(ref_logits)).abs().max()) < (1e-4 if dtype == torch.float32 else 1e-2)


def test_logits_mode_with_an_outside_criterion_gives_the_same_gradients():
    P = O.make_params(CFG, seed=3)
    b = _batch("1d")
    m = _model(torch.float32, P)
    logits = m(*_inputs(b))
    assert tuple(logits.shape) == (4, C) and logits.requires_grad and logits.dtype == torch.float32
    criterion = torch.nn.BCEWithLogitsLoss(pos_weight=POS_W.to(DEV))         # main.py:93-101, 213-216
    criterion(logits, b["labels"].to(DEV)).backward()
    g1 = {k: v.clone() for k, v in _grads(m).items()}
    m.zero_grad()
    m(*_inputs(b), labels=b["labels"].to(DEV)).backward()
    _compare_grads(_grads(m), {k: v.cpu() for k, v in g1.items()}, 1e-4)
    m.set_pos_weight(None)                       # without pos_weight: plain BCEWithLogitsLoss
    l0 = m(*_inputs(b), labels=b["labels"].to(DEV))
    ref0, _, _ = _reference(P, _head(m), b, pos_weight=None)
    assert abs(float(l0.detach()) - ref0) < 1e-4


def test_compact_tail_equals_a_run_over_full_rows():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    m = _model(torch.float32, P)
    loss = m(*_inputs(b), labels=b["labels"].to(DEV))
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.bert.named_parameters() if not k.startswith("enc.pooler.")}
    eng = m.bert.engine
    cls_tok, txt, mask, seg, (feats, pos), sep = _inputs(b)
    eng.training, eng.keep_acts = False, True
    hidden, _ = eng.encoder_forward(cls_tok, txt, mask, seg, feats, pos, sep, tail_rows=None)
    assert tuple(hidden.shape) == (4, eng.S["L"], CFG.hidden)
    v = hidden[:, 0].detach().clone().requires_grad_(True)
    pw, pb = (m.bert.get_parameter(f"enc.pooler.dense.{n}").detach() for n in ("weight", "bias"))
    hd = _head(m)
    full_loss = F.binary_cross_entropy_with_logits(F.linear(torch.tanh(F.linear(v, pw, pb)), hd["clf.weight"], hd["clf.bias"]),
                                                   b["labels"].to(DEV), pos_weight=POS_W.to(DEV))
    full_loss.backward()
    assert abs(float(full_loss) - float(loss)) < 1e-6
    eng.zero_grad()
    dh = eng._buf("dhidden", (eng.S["M"], CFG.hidden), eng.adt)
    dh.zero_()
    dh.view(4, -1, CFG.hidden)[:, 0] = v.grad
    eng.S["dhidden"] = dh
    eng.encoder_backward()
    _compare_grads(got, {k: eng.g[k].clone().cpu() for k in got}, 1e-4)


@pytest.mark.parametrize("family", ["s2s", "full", "1d"])
def test_packed_and_padded_runs_agree(family):
    P = O.make_params(CFG, seed=3)
    b = _batch(family, B=8, seed=21)
    m = _model(torch.bfloat16, P, seed=9)
    l1 = m(*_inputs(b), labels=b["labels"].to(DEV))
    l1.backward()
    g1 = {k: v.float().clone() for k, v in _grads(m).items()}
    p1 = m.predict(*_inputs(b))
    m.zero_grad()
    desc = mv.data.MaskDesc.make(family, 16, 45, b["n_ids"], DEV)
    l2 = m(*_inputs(b, desc), labels=b["labels"].to(DEV))
    l2.backward()
    assert abs(float(l1) - float(l2)) < 1e-3 * max(1.0, float(l1))
    _compare_grads(_grads(m), {k: v.cpu() for k, v in g1.items()}, 3e-2)
    assert float((p1 - m.predict(*_inputs(b, desc))).abs().max()) < 1e-2


def test_bert_base_16bit_loss_matches_fp32():
    cfg = O.CONFIGS["base"]
    P = O.make_params(cfg, seed=2)
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(cfg, 4, 256, 253, "1d", seed=4).items()}
    t = _labels(4, 4)
    losses = []
    for dtype in (torch.float32, torch.bfloat16):
        m = _model(dtype, P, seed=1, cfg=cfg)
        loss = m(*_inputs(b), labels=t.to(DEV))
        loss.backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        losses.append(float(loss))
        del m
        torch.cuda.empty_cache()
    assert abs(losses[0] - losses[1]) < 1e-2, losses


def test_save_load_round_trip_and_pretraining_checkpoint(tmp_path):
    P = O.make_params(CFG, seed=3)
    b = _batch("full")
    m = _model(torch.bfloat16, P)
    m.save_pretrained(str(tmp_path / "clf"))
    m2 = mv.CXRBertForClassification.from_pretrained(str(tmp_path / "clf"), dtype=torch.bfloat16, device=DEV)
    assert m2.n_classes == C
    m2.eval()
    assert torch.equal(m.predict(*_inputs(b)), m2.predict(*_inputs(b)))
    pre = mv.CXRBERT(_cfg_dict(CFG), None, dtype=torch.bfloat16, device=DEV)
    pre.load_state_dict(P)
    pre.save_pretrained(str(tmp_path / "pre"))
    m3 = mv.CXRBertForClassification.from_pretrained(str(tmp_path / "pre"), n_classes=C, dtype=torch.bfloat16, device=DEV)
    assert torch.equal(m3.bert.engine.flat_p, pre.engine.flat_p) and bool(torch.isfinite(m3.predict(*_inputs(b))).all())


def _groups(model):
    """get_optimizer's grouping (main.py:115-120)."""
    named = list(model.named_parameters())
    return [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
            {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]


def test_short_finetune_with_bertadam_reaches_micro_f1_one():
    """8 synthetic samples that share their findings (classes 0-4 present, 5-13 absent: what a randomly initialised encoder can
    learn in a few steps, as test_vqa_gpu's fine-tune), optim.BertAdam with the reference's groups and warmup = 0.1, until the
    micro-F1 from the device counters is 1; capped at 60 steps = 2 x the 30 of test_vqa_gpu's fine-tune (zero-lr first step, warm-up)."""
    P = O.make_params(CFG, seed=3)
    b = _batch("1d", B=8, seed=31)
    t = torch.zeros(8, C)
    t[:, :5] = 1.0
    m = _model(torch.bfloat16, P, pos_weight=None)
    m.train()
    cap = 60
    opt = mv.optim.BertAdam(_groups(m), lr=2e-3, warmup=0.1, t_total=cap)
    first, used = None, cap
    for s in range(cap):
        opt.zero_grad()
        m.reset_stats()
        loss = m(*_inputs(b), labels=t.to(DEV))
        loss.backward()
        opt.step()
        first = float(loss) if first is None else first
        if metrics(torch.zeros(8, C), t, counters=m.clf_stats)["micro_f1"] == 1.0 and s > 0:
            used = s + 1
            break
    m.eval()
    m.reset_stats()
    with torch.no_grad():
        loss = m(*_inputs(b), labels=t.to(DEV))
    res = metrics(m.predict(*_inputs(b)), t, counters=m.clf_stats)
    print(f"clf fine-tune: {used} steps, loss {first:.4f} -> {float(loss):.4f}, micro-F1 {res['micro_f1']:.3f}")
    assert res["micro_f1"] == 1.0 and float(loss) < first
    for k, p in m.bert.named_parameters():       # unreached heads: bit-unchanged under BertAdam
        if k.startswith(("mlm.", "itm.")):
            assert torch.equal(p.detach().cpu(), P[k].float()), k


def test_overflowed_backward_is_redone_with_a_smaller_scale():
    """f16 gradient operands under a loss scale far past f16's range: the backward overflows (the head's gradients included), redoes
    itself with S / 16 until everything is finite and hands over the gradients of a twin run at the default scale."""
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    grads = []
    for scale in (2.0 ** 40, None):
        m = _model(torch.bfloat16, P)
        eng = m.bert.engine
        assert eng.scaler is not None
        loss = m(*_inputs(b), labels=b["labels"].to(DEV))
        if scale is not None:
            eng.reset_scaler(scale)
        loss.backward()
        if scale is not None:
            assert float(eng.scaler[0]) < scale                      # the redo did happen
        grads.append({k: g.detach().float().cpu() for k, g in _grads(m).items()})
    got, twin = grads
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    off = ("itm.", "mlm.")                                            # as the oracle test: no gradient reaches them
    for k, g in got.items():
        if k.startswith(off):
            assert float(g.abs().max()) == 0.0, k
    _compare_grads(got, {k: g for k, g in twin.items() if not k.startswith(off)}, 3e-2)
