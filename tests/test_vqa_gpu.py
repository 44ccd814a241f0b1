"""VQA fine-tuning and answer prediction on the MI355X: the kernels of csrc/mv_vqa.hip (and the BIAS_RELU / ReLU-backward additions)
against torch, and CXRBertForVQA against the oracle encoder (oracle/cxrbert_oracle.py, CPU autograd) + a torch classifier +
BCEWithLogitsLoss -- the reference's BertForPreTrainingLossMask(tasks='vqa') arithmetic on CXRBERT."""
import pytest
import torch
import torch.nn.functional as F

import medvill_amd as mv
from medvill_amd import hip_ops as ops
from medvill_amd._lib import EPI_BIAS_RELU
from oracle import cxrbert_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 458


def _cfg_dict(c):
    return dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)


def _targets(B, seed, A=A):
    """Soft targets as data_loader.py:255-272 builds them (target.scatter_(0, labels, scores)) and answer types 0 / 1 / other."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(B, A)
    for b in range(B):
        k = int(torch.randint(1, 4, (1,), generator=g))
        idx = torch.randperm(A, generator=g)[:k]
        t[b, idx] = torch.tensor([1.0, 0.6, 0.3])[:k]
    types = torch.tensor([b % 3 for b in range(B)], dtype=torch.int64)     # 0 CLOSED, 1 OPEN, 2 neither
    return t, types


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16, torch.float16])
def test_bce_fwd_bwd_matches_torch(gdt):
    g = torch.Generator().manual_seed(7)
    R, Ap = 37, 464
    z = torch.randn(R, Ap, generator=g) * 3
    z[0, 5] = z[0, 9] = 50.0                       # tie: both argmaxes pick the lower column
    z[1, 0] = 60.0                                 # column 0 wins training, not inference
    z[2, :A] = 0.0                                 # all equal: training 0, inference 1
    z[3, :40] = 80.0
    z[3, 40:A] = -80.0                             # saturated logits: finite loss, exact gradients
    y, types = _targets(R, 3)
    zd, yd = z.to(DEV), y.to(DEV)
    stats = torch.zeros(6, device=DEV)
    d = torch.full((R, Ap), 7.0, device=DEV).to(gdt)
    at, ai = torch.empty(R, dtype=torch.int64, device=DEV), torch.empty(R, dtype=torch.int64, device=DEV)
    S = torch.tensor([4.0], device=DEV)
    ops.bce_fwd_bwd(zd, A, ld=Ap, target=yd, ans_type=types.to(DEV, torch.int32), stats=stats, dgrad=d, ldd=Ap, grad_scale=0.5,
                    loss_scale_dev=S, arg_train=at, arg_infer=ai)
    zz = z[:, :A].double()
    loss = F.binary_cross_entropy_with_logits(zz, y.double(), reduction="sum")
    grad = (torch.sigmoid(zz) - y.double()) * 0.5 * 4.0
    ref_at = torch.max(z[:, :A], 1)[1]
    ref_ai = torch.max(z[:, 1:A], 1)[1] + 1
    assert torch.equal(at.cpu(), ref_at) and torch.equal(ai.cpu(), ref_ai)
    assert int(at[0]) == 5 and int(ai[0]) == 5 and int(at[1]) == 0 and int(at[2]) == 0 and int(ai[2]) == 1
    st = stats.double().cpu()
    assert torch.isfinite(st).all()
    assert abs(float(st[1]) - float(loss)) < 1e-5 * float(loss)
    score = y[torch.arange(R), ref_at].double()
    assert abs(float(st[0]) - float(score.sum())) < 1e-5
    for k, ty in ((2, 0), (4, 1)):
        sel = types == ty
        assert abs(float(st[k]) - float(score[sel].sum())) < 1e-5 and float(st[k + 1]) == float(sel.sum())
    tol = 1e-6 if gdt == torch.float32 else (2e-2 if gdt == torch.bfloat16 else 3e-3)
    assert float((d[:, :A].double().cpu() - grad).abs().max()) < tol * 2.0
    assert float(d[:, A:].float().abs().max()) == 0.0          # padding columns written as zero
    # inference form: no target, no loss, no gradient
    ai2 = torch.empty(R, dtype=torch.int64, device=DEV)
    ops.bce_fwd_bwd(zd, A, ld=Ap, arg_infer=ai2)
    assert torch.equal(ai2.cpu(), ref_ai)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [3, 64, 256])
def test_gemm_rows_bias_relu(dt, M):
    g = torch.Generator().manual_seed(M)
    K, N = 256, 464
    x = torch.randn(M, K, generator=g).to(DEV, dt)
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV, dt)
    b = torch.randn(N, generator=g).to(DEV) * 0.3
    c = torch.empty(M, N, device=DEV, dtype=dt)
    ops.gemm_rows(x, w, c, M=M, N=N, K=K, bias=b, epi=EPI_BIAS_RELU)
    ref = torch.relu(x.float() @ w.float().t() + b)
    tol = 2e-2 if dt == torch.bfloat16 else 4e-3
    assert float((c.float() - ref).abs().max()) < tol * max(1.0, float(ref.abs().max()))
    assert float(c.float().min()) >= 0.0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_dact_relu_and_rows_mul(dt):
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(33, 256, generator=g).to(DEV, dt)
    y = torch.relu(torch.randn(33, 256, generator=g)).to(DEV, dt)
    out = torch.empty_like(dy)
    ops.dact(2, dy, y, out, dy.numel())
    assert torch.equal(out.float(), dy.float() * (y.float() > 0))
    src = torch.randn(20, 128, generator=g).to(DEV, dt)
    ra = torch.tensor([3, 19, 0, 7, -1], dtype=torch.int32, device=DEV)
    rb = torch.tensor([1, 1, 12, 7, 2], dtype=torch.int32, device=DEV)
    o = torch.full((5, 128), 9.0, device=DEV).to(dt)
    ops.rows_mul(src, ra, src, rb, o, R=5, H=128)
    ref = src[ra[:4].long()].float() * src[rb[:4].long()].float()
    assert float((o[:4].float() - ref).abs().max()) <= (0 if dt == torch.float32 else 1e-2) * float(ref.abs().max()) + 1e-6
    assert float(o[4].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ model against the oracle
CFG = O.CONFIGS["c1"]
FAMILIES = ["full", "s2s", "bar", "1d"]


def _batch(family, B=4, N=16, S=45, seed=11):
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, B, N, S, family, seed=seed).items()}
    t, ty = _targets(B, seed)
    b["target"], b["ans_type"] = t, ty
    return b


def _model(dtype, P, seed=5, head_scale=1.0):
    m = mv.CXRBertForVQA(_cfg_dict(CFG), dtype=dtype, device=DEV)
    m.bert.load_state_dict(P, strict=True)
    m.reset_head(seed=seed)
    if head_scale != 1.0:                      # spread the answer logits (argmax comparisons need margins above 16-bit rounding)
        with torch.no_grad():
            for p in m.ans_classifier.parameters():
                p.mul_(head_scale)
    m.eval()
    return m


def _inputs(b, mask=None):
    return (b["cls_tok"].to(DEV), b["input_txt"].to(DEV), b["attn_mask"].to(DEV) if mask is None else mask, b["segment"].to(DEV),
            (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))


def _reference(P, head, b, infer=False):
    """oracle encoder (CPU, f32 autograd) + torch classifier + BCEWithLogitsLoss (model.py:1016-1022) -> loss, grads; or, with
    `infer`, the logits of [CLS] (.) image [SEP] (model.py:979-983)."""
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    hg = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in head.items()}
    x, _ = O.encode(Pg, CFG, b["cls_tok"], b["input_txt"], b["attn_mask"], b["segment"], b["img_feats"], b["img_pos"], b["sep_tok"])
    N = b["img_feats"].shape[1]
    v = x[:, 0] * x[:, N + 1] if infer else x[:, 0]
    h = torch.relu(F.linear(v, hg["ans_classifier.0.weight"], hg["ans_classifier.0.bias"]))
    logits = F.linear(h, hg["ans_classifier.2.weight"], hg["ans_classifier.2.bias"])
    if infer:
        return logits.detach()
    loss = F.binary_cross_entropy_with_logits(logits, b["target"])
    loss.backward()
    grads = {k: p.grad for k, p in Pg.items() if p.grad is not None}
    grads.update({k: p.grad for k, p in hg.items()})
    return float(loss.detach()), grads, logits.detach()


def _head(m):
    return {k: p.detach() for k, p in m.ans_classifier.named_parameters(prefix="ans_classifier")}


def _grads(m):
    out = {k: p.grad for k, p in m.bert.named_parameters()}
    out.update({k: p.grad for k, p in m.ans_classifier.named_parameters(prefix="ans_classifier")})
    return out


def _compare_grads(got, ref, rtol):
    gmax = max(float(g.abs().max()) for g in ref.values())
    floor = (1e-5 if rtol < 1e-3 else 3e-2) * gmax
    for k, r in ref.items():
        g = got[k].float().cpu()
        n = r.double().norm()
        e1 = float((g.double() - r.double()).norm()) / max(float(n), floor * r.numel() ** 0.5)
        assert e1 < rtol, (k, e1, float(n))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype,ltol,rtol", [(torch.float32, 1e-4, 2e-4), (torch.bfloat16, 1e-2, 3e-2)])
def test_vqa_loss_and_every_gradient_match_the_oracle(family, dtype, ltol, rtol):
    P = O.make_params(CFG, seed=3)
    b = _batch(family)
    m = _model(dtype, P)
    _, loss = m(*_inputs(b), ans_labels=b["target"].to(DEV), ans_type=b["ans_type"].to(DEV))
    loss.backward()
    ref_loss, ref_g, ref_logits = _reference(P, _head(m), b)
    assert abs(float(loss.detach()) - ref_loss) < ltol, (float(loss.detach()), ref_loss)
    _compare_grads(_grads(m), ref_g, rtol)
    # the pooler, ITM and MLM heads get no gradient (the VQA model has none of them)
    for k, p in m.bert.named_parameters():
        if k.startswith(("enc.pooler.", "itm.", "mlm.")):
            assert float(p.grad.abs().max()) == 0.0, k
    # statistics: score = one_hot(argmax) . target, split by answer type
    st = m.vqa_stats.cpu()
    am = ref_logits.argmax(1)
    if dtype == torch.float32:
        score = b["target"][torch.arange(4), am]
        assert abs(float(st[0]) - float(score.sum())) < 1e-6
        assert float(st[3]) == float((b["ans_type"] == 0).sum()) and float(st[5]) == float((b["ans_type"] == 1).sum())
    assert abs(float(st[1]) / (4 * A) - float(loss)) < 1e-6


def test_logits_mode_is_differentiable_and_matches_the_loss_mode():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    m = _model(torch.float32, P)
    logits = m(*_inputs(b))
    assert tuple(logits.shape) == (4, A) and logits.requires_grad
    F.binary_cross_entropy_with_logits(logits, b["target"].to(DEV)).backward()
    g1 = {k: v.clone() for k, v in _grads(m).items()}
    m.zero_grad()
    _, loss = m(*_inputs(b), ans_labels=b["target"].to(DEV))
    loss.backward()
    _compare_grads(_grads(m), {k: v.cpu() for k, v in g1.items()}, 1e-4)


def test_compact_tail_R0_equals_a_run_over_full_rows():
    """The classifier reads the [CLS] rows only: the engine's last layer runs on those B rows (tail_rows = [], the R = 0 corner of the
    fused step's tail path).  Same loss and encoder gradients as the encoder over all rows with the gradient scattered to rows b*L."""
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    m = _model(torch.float32, P)
    _, loss = m(*_inputs(b), ans_labels=b["target"].to(DEV))
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.bert.named_parameters()}
    eng = m.bert.engine
    cls_tok, txt, mask, seg, (feats, pos), sep = _inputs(b)
    eng.training, eng.keep_acts = False, True
    hidden, _ = eng.encoder_forward(cls_tok, txt, mask, seg, feats, pos, sep, tail_rows=None)
    assert tuple(hidden.shape) == (4, eng.S["L"], CFG.hidden)
    v = hidden[:, 0].detach().clone().requires_grad_(True)
    hd = {k: p.detach().clone().requires_grad_(True) for k, p in _head(m).items()}
    h = torch.relu(F.linear(v, hd["ans_classifier.0.weight"], hd["ans_classifier.0.bias"]))
    full_loss = F.binary_cross_entropy_with_logits(F.linear(h, hd["ans_classifier.2.weight"], hd["ans_classifier.2.bias"]),
                                                   b["target"].to(DEV))
    full_loss.backward()
    assert abs(float(full_loss) - float(loss)) < 1e-6
    eng.zero_grad()
    dh = eng._buf("dhidden", (eng.S["M"], CFG.hidden), eng.adt)
    dh.zero_()
    dh.view(4, -1, CFG.hidden)[:, 0] = v.grad
    eng.S["dhidden"] = dh
    eng.encoder_backward()
    ref = {k: eng.g[k].clone() for k in got}
    _compare_grads(got, {k: v_.cpu() for k, v_ in ref.items()}, 1e-4)


@pytest.mark.parametrize("family", ["s2s", "full", "1d"])
def test_packed_and_padded_runs_agree(family):
    P = O.make_params(CFG, seed=3)
    b = _batch(family, B=8, seed=21)
    m = _model(torch.bfloat16, P, seed=9, head_scale=30.0)
    _, l1 = m(*_inputs(b), ans_labels=b["target"].to(DEV))
    l1.backward()
    g1 = {k: v.float().clone() for k, v in _grads(m).items()}
    a1 = m.predict(*_inputs(b))
    m.zero_grad()
    desc = mv.data.MaskDesc.make(family, 16, 45, b["n_ids"], DEV)
    _, l2 = m(*_inputs(b, desc), ans_labels=b["target"].to(DEV))
    l2.backward()
    assert abs(float(l1) - float(l2)) < 1e-3 * max(1.0, float(l1))
    _compare_grads(_grads(m), {k: v.cpu() for k, v in g1.items()}, 3e-2)
    a2 = m(*_inputs(b, desc), vqa_inference=True)
    logits = _reference(P, _head(m), b, infer=True)
    top2 = torch.topk(logits[:, 1:], 2, dim=-1).values
    sure = ((top2[:, 0] - top2[:, 1]) > 0.05 * logits.std(dim=1)).to(DEV)
    assert torch.equal(a1[sure], a2[sure])
    with torch.no_grad():                      # the [CLS] logits themselves
        z1, z2 = m(*_inputs(b)), m(*_inputs(b, desc))
    assert float((z1 - z2).abs().max()) < 2e-2 * max(1.0, float(z1.abs().max()))


@pytest.mark.parametrize("family", ["s2s", "full", "bar"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inference_argmax_of_cls_times_sep(family, dtype):
    P = O.make_params(CFG, seed=3)
    b = _batch(family, B=8, seed=21)
    m = _model(dtype, P, seed=9, head_scale=30.0)
    with torch.no_grad():
        ans = m(*_inputs(b), vqa_inference=True).cpu()
    logits = _reference(P, _head(m), b, infer=True)
    ref = torch.max(logits[:, 1:], -1)[1] + 1
    if dtype == torch.float32:
        assert torch.equal(ans, ref)
    else:
        # 16-bit: the chosen answer's reference logit is within the 16-bit tolerance of the best one, and rows whose top-2 margin
        # exceeds that tolerance pick exactly the reference answer
        tol = 1e-2 * float(logits.abs().max())
        top2 = torch.topk(logits[:, 1:], 2, dim=-1).values
        assert bool((logits.gather(1, ans.view(-1, 1)).view(-1) >= top2[:, 0] - tol).all())
        sure = (top2[:, 0] - top2[:, 1]) > tol
        assert torch.equal(ans[sure], ref[sure])
    assert int(ans.min()) >= 1 and int(ans.max()) < A


def test_bert_base_16bit_loss_matches_fp32():
    cfg = O.CONFIGS["base"]
    P = O.make_params(cfg, seed=2)
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(cfg, 4, 256, 253, "s2s", seed=4).items()}
    t, ty = _targets(4, 4)
    losses = []
    for dtype in (torch.float32, torch.bfloat16):
        m = mv.CXRBertForVQA(_cfg_dict(cfg), dtype=dtype, device=DEV)
        m.bert.load_state_dict(P, strict=True)
        m.reset_head(seed=1)
        m.eval()
        _, loss = m(*_inputs(b), ans_labels=t.to(DEV), ans_type=ty.to(DEV))
        loss.backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        losses.append(float(loss))
        del m
        torch.cuda.empty_cache()
    assert abs(losses[0] - losses[1]) < 1e-2, losses


# ------------------------------------------------------------------------------------------------ optimizer and fine-tuning
class _TorchHFAdamW(torch.optim.Optimizer):
    """A plain torch optimizer with the update rule of medvill_amd.optim.AdamW (HF AdamW, oracle.hf_adamw_step: eps added to sqrt(v)
    before the bias correction -- torch.optim.AdamW adds it after, which differs wherever |g| is near eps)."""

    def __init__(self, params, lr):
        super().__init__(params, dict(lr=lr))
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        for p in self.param_groups[0]["params"]:
            st = self.state[p]
            if not st:
                st["m"], st["v"] = torch.zeros_like(p), torch.zeros_like(p)
            O.hf_adamw_step(p, p.grad, st["m"], st["v"], self.t, lr=self.param_groups[0]["lr"])


def test_fused_adamw_over_the_vqa_model_equals_a_torch_optimizer():
    """medvill_amd.optim.AdamW(vqa.parameters()): the encoder's flat buffer and the classifier's (one more fused launch) against a torch
    optimizer over the same Parameters, 3 steps; and torch.optim.AdamW itself runs on vqa.parameters()."""
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    ms = [_model(torch.bfloat16, P) for _ in range(3)]
    lr = 1e-4
    opts = [mv.optim.AdamW(ms[0].parameters(), lr=lr), _TorchHFAdamW(ms[1].parameters(), lr=lr),
            torch.optim.AdamW(ms[2].parameters(), lr=lr, weight_decay=0.0, eps=1e-6)]
    assert opts[0]._task is ms[0]
    start = ms[2].ans_classifier[2].weight.detach().clone()
    for _ in range(3):
        for m, opt in zip(ms, opts):
            opt.zero_grad()
            _, loss = m(*_inputs(b), ans_labels=b["target"].to(DEV))
            loss.backward()
            opt.step()
    p0 = dict(ms[0].named_parameters())
    for k, p in ms[1].named_parameters():
        d = (p0[k].detach() - p.detach()).abs()
        # f32 atomics of the embedding backward are not reproducible, and Adam turns a near-zero gradient into a step of ~lr
        assert float(d.max()) <= 6 * lr + 1e-7, k
        assert float((d > 0.1 * lr).float().mean()) < 5e-2, k
    assert float((p0["ans_classifier.2.weight"].detach() - ms[1].ans_classifier[2].weight.detach()).abs().max()) < 0.1 * lr
    moved = (ms[2].ans_classifier[2].weight.detach() - start).abs()
    assert bool(torch.isfinite(moved).all()) and float(moved.max()) > 0.5 * lr
    assert all(bool(torch.isfinite(p).all()) for p in ms[2].parameters())


def test_short_finetune_drives_the_loss_down_and_the_score_to_one():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s", B=8, seed=31)
    # closed questions sharing the answer 5 (score 1) with a weaker per-question alternative (score 0.3): under the s2s mask the [CLS]
    # rows of a randomly initialised encoder are nearly identical across samples, so what 30 steps can learn is the shared answer
    t = torch.zeros(8, A)
    t[torch.arange(8), torch.arange(8) * 37 + 9] = 0.3
    t[:, 5] = 1.0
    m = _model(torch.bfloat16, P)
    m.train()
    opt = mv.optim.AdamW(m.parameters(), lr=2e-3, weight_decay=0.0)
    first = None
    for _ in range(30):
        opt.zero_grad()
        _, loss = m(*_inputs(b), ans_labels=t.to(DEV), ans_type=torch.zeros(8, dtype=torch.int64))
        loss.backward()
        opt.step()
        first = float(loss) if first is None else first
    m.eval()
    with torch.no_grad():
        _, loss = m(*_inputs(b), ans_labels=t.to(DEV), ans_type=torch.zeros(8, dtype=torch.int64))
    assert float(loss) < 0.5 * first
    assert float(m.vqa_stats[0]) == 8.0 and float(m.vqa_stats[2]) == 8.0 and float(m.vqa_stats[3]) == 8.0


def test_no_grad_forward_keeps_no_activations():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    m = _model(torch.bfloat16, P)
    with torch.no_grad():
        _, loss = m(*_inputs(b), ans_labels=b["target"].to(DEV))
        logits = m(*_inputs(b))
    eng = m.bert.engine
    assert eng.S["keep"] is False and loss.grad_fn is None and logits.grad_fn is None
    assert "qkv0" not in eng._ws and "qkv_nk" in eng._ws            # one shared scratch set, no per-layer activations


def test_overflowed_backward_is_redone_with_a_smaller_scale():
    """f16 gradient operands under a loss scale far past f16's range: the backward overflows (the classifier's gradients included),
    redoes itself with S / 16 until everything is finite and hands over the gradients of a twin run at the default scale."""
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    grads = []
    for scale in (2.0 ** 40, None):
        m = _model(torch.bfloat16, P)
        eng = m.bert.engine
        assert eng.scaler is not None
        _, loss = m(*_inputs(b), ans_labels=b["target"].to(DEV), ans_type=b["ans_type"].to(DEV))
        if scale is not None:
            eng.reset_scaler(scale)
        loss.backward()
        if scale is not None:
            assert float(eng.scaler[0]) < scale                      # the redo did happen
        grads.append({k: g.detach().float().cpu() for k, g in _grads(m).items()})
    got, twin = grads
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    off = ("enc.pooler.", "itm.", "mlm.")                             # as the oracle test: no gradient reaches them
    for k, g in got.items():
        if k.startswith(off):
            assert float(g.abs().max()) == 0.0, k
    _compare_grads(got, {k: g for k, g in twin.items() if not k.startswith(off)}, 3e-2)
