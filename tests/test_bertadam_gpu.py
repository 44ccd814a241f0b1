"""BertAdam on the MI355X: mv_tensor_sqnorms and mv_bertadam_step (csrc/mv_optim.hip) against tests/golden/bertadam.npz -- the
reference's own optimizer stepped over a recorded gradient sequence (tools/gen_bertadam_golden.py) -- and medvill_amd.optim.BertAdam
over CXRBERT and CXRBertForVQA against a plain-torch transcription of the update rule.

Tolerance of the fixture comparison: 2e-6 max-abs on the parameters, the margin tests/test_kernels_gpu.py::test_adamw_known_answer grants
mv_adamw_step against adamw.npz.  The only legitimate difference is the summation order of the gradient norm that enters the clip
factor; the fixture records the reference's own spread between an f32 and an f64 norm (`clip_spread`, 1.2e-7), well inside it, so the
clip cases get no extra margin."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import medvill_amd as mv
from medvill_amd import _lib
from medvill_amd import hip_ops as ops
from medvill_amd.engine import ModelConfig, param_layout
from medvill_amd.optim import build_tables
from oracle import cxrbert_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-6          # test_adamw_known_answer's margin


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "bertadam.npz"))


def _dev_tables(entries):
    t, c = build_tables(entries)
    return t.to(DEV), c.to(DEV)


def _sqnorms(x, tensors, chunks):
    part = torch.full((chunks.numel(),), 7.0, device=DEV)
    out = torch.full((tensors.shape[0],), 7.0, device=DEV)
    ops.tensor_sqnorms(x, tensors, chunks, part, out)
    return out


# ------------------------------------------------------------------------------------------------ mv_tensor_sqnorms
def test_sqnorms_on_the_bert_base_layout_and_bit_reproducible():
    lay, n = param_layout(ModelConfig())          # BERT-base: tensors of 2 (itm.linear.bias) to 23 M elements (word embeddings)
    sizes = [math.prod(s) for _, s in lay.values()]
    assert min(sizes) == 2 and max(sizes) > 20_000_000
    entries = [(off, math.prod(shape), False, True) for off, shape in lay.values()]
    tensors, chunks = _dev_tables(entries)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(n, generator=g, device=DEV) * 0.02
    a = _sqnorms(x, tensors, chunks)
    b = _sqnorms(x, tensors, chunks)
    assert torch.equal(a, b)                                          # same bits: fixed summation order, no atomics
    ref = torch.stack([x[off:off + cnt].double().pow(2).sum() for off, cnt, _, _ in entries])
    # f32 accumulation: an element passes through at most 16 + 6 + 4 + 90 + 6 additions (thread, wave, block, lane over <= 5,723
    # partials, wave) of non-negative terms: relative error <= 122 * 2^-24 = 7.3e-6
    rel = ((a.double() - ref).abs() / ref).max()
    assert float(rel) < 1e-5, float(rel)


def test_sqnorms_on_the_fixture_sizes_masks_the_gaps_and_skips_inactive(fx):
    offs, sizes = fx["offsets"].tolist(), fx["sizes"].tolist()
    n = int(fx["p0"].shape[0])
    x = torch.from_numpy(fx["grads"][0]).to(DEV).clone()
    covered = torch.zeros(n, dtype=torch.bool)
    for o, s in zip(offs, sizes):
        covered[o:o + s] = True
    x[~covered.to(DEV)] = 1e3                                         # the alignment gaps must not enter any norm
    entries = [(o, s, False, i != 2) for i, (o, s) in enumerate(zip(offs, sizes))]
    out = _sqnorms(x, *_dev_tables(entries))
    for i, (o, s) in enumerate(zip(offs, sizes)):
        ref = float(x[o:o + s].double().pow(2).sum())
        if i == 2:
            assert float(out[i]) == 0.0
        else:
            assert abs(float(out[i]) - ref) <= 1e-5 * ref, (i, float(out[i]), ref)


def test_sqnorms_of_a_tensor_that_spans_two_chunks(fx):
    offs, sizes = fx["big/offsets"].tolist(), fx["big/sizes"].tolist()
    assert sizes[0] > ops.OPTIM_CHUNK and sizes[0] % 4 == 3
    x = torch.from_numpy(fx["big/grads"][0]).to(DEV).clone()
    x[offs[0] + sizes[0]:offs[1]] = 1e3                                # the gap behind the 3-element tail
    out = _sqnorms(x, *_dev_tables([(o, s, False, True) for o, s in zip(offs, sizes)]))
    for i, (o, s) in enumerate(zip(offs, sizes)):
        ref = float(x[o:o + s].double().pow(2).sum())
        assert abs(float(out[i]) - ref) <= 1e-5 * ref, (i, float(out[i]), ref)


# ------------------------------------------------------------------------------------------------ mv_bertadam_step
def _run_case(fx, name, shadows=False, scaler=None):
    pre = "big/" if name == "big" else ""              # `big` has a layout of its own: a tensor that spans two chunks
    offs, sizes, decay = fx[pre + "offsets"].tolist(), fx[pre + "sizes"].tolist(), fx[pre + "decay"].tolist()
    lr, warmup, t_total, b1, b2, e, wd, mgn = [float(v) for v in fx[f"{name}/hyper"]]
    none = int(fx["none_grad"]) if name == "none_grad" else -1
    tensors, chunks = _dev_tables([(o, s, d, i != none) for i, (o, s, d) in enumerate(zip(offs, sizes, decay))])
    if name == "big":
        assert chunks.tolist() == [0, 0, 1] and tensors[1].tolist()[2] == 2
    p = torch.from_numpy(fx[pre + "p0"]).to(DEV).clone()
    n = p.numel()
    covered = torch.zeros(n, dtype=torch.bool, device=DEV)
    for o, s in zip(offs, sizes):
        covered[o:o + s] = True
    p[~covered] = 3.25                                                # sentinels in the gaps
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sh = torch.full((n,), 9.0, device=DEV).to(torch.bfloat16) if shadows else None
    shf = torch.full((n,), 9.0, device=DEV).to(torch.float16) if shadows else None
    part, sq = torch.zeros(chunks.numel(), device=DEV), torch.zeros(len(sizes), device=DEV)
    worst = 0.0
    steps = fx[f"{name}/p"].shape[0]
    for s in range(steps):
        g = torch.from_numpy(fx[pre + "grads"][s]).to(DEV).clone()
        g[~covered] = 1e3
        g0 = g.clone()
        if mgn > 0:
            ops.tensor_sqnorms(g, tensors, chunks, part, sq)
        ops.bertadam_step(p, g, m, v, tensors, chunks, sq if mgn > 0 else None, lr=lr, step=s, warmup=warmup, t_total=int(t_total),
                          schedule=str(fx[f"{name}/schedule"]), b1=b1, b2=b2, eps=e, weight_decay=wd, max_grad_norm=mgn, shadow=sh,
                          shadow_f16=shf, scaler_state=scaler)
        assert torch.equal(g, g0)                                     # the stored gradient is left unclipped
        ref = torch.from_numpy(fx[f"{name}/p"][s]).to(DEV)
        err = float((p - ref)[covered].abs().max())
        worst = max(worst, err)
        print(f"bertadam fixture {name} step {s}: max |p - ref| = {err:.3e}")
        assert err < TOL, (name, s, err)
        assert bool((p[~covered] == 3.25).all())                      # gaps untouched
    if name == "big":                                   # (the fixture holds no moments for it: step 1's enter step 2's parameters)
        print(f"bertadam fixture {name}: worst p {worst:.3e}")
        return p, m, v, sh, shf, covered
    em = float((m - torch.from_numpy(fx[f"{name}/m"]).to(DEV))[covered].abs().max())
    ev = float((v - torch.from_numpy(fx[f"{name}/v"]).to(DEV))[covered].abs().max())
    print(f"bertadam fixture {name}: worst p {worst:.3e}, m {em:.3e}, v {ev:.3e}")
    assert em < TOL and ev < TOL
    assert bool((m[~covered] == 0).all()) and bool((v[~covered] == 0).all())
    return p, m, v, sh, shf, covered


@pytest.mark.parametrize("case", ["main", "none_grad", "const_lr", "noclip", "constant", "cosine", "big"])
def test_bertadam_step_against_the_reference_fixture(fx, case):
    p, m, v, _, _, _ = _run_case(fx, case)
    if case == "main":
        # step 0 under warm-up moved nothing (lr_t = 0) but updated the moments -- the fixture's first row says so itself
        o, s = int(fx["offsets"][3]), int(fx["sizes"][3])
        assert np.array_equal(fx["main/p"][0][o:o + s], fx["p0"][o:o + s])
    if case == "none_grad":
        i = int(fx["none_grad"])
        o, s = int(fx["offsets"][i]), int(fx["sizes"][i])
        assert torch.equal(p[o:o + s].cpu(), torch.from_numpy(fx["p0"][o:o + s]))          # bit-unchanged
        assert float(m[o:o + s].abs().max()) == 0.0 and float(v[o:o + s].abs().max()) == 0.0


def test_cosine_after_the_warmup_follows_the_formula(fx):
    """The reference's warmup_cosine cannot run past its warm-up (torch.cos of a Python float raises), so the branch is checked against
    0.5 (1 + cos(pi x)): with b1 = b2 = 0, e = 0 and no decay the update is lr_t * sign(g)."""
    n = 64
    tensors, chunks = _dev_tables([(0, n, False, True)])
    p, m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    g = torch.ones(n, device=DEV)
    ops.bertadam_step(p, g, m, v, tensors, chunks, None, lr=1.0, step=5, warmup=0.25, t_total=8, schedule="warmup_cosine", b1=0.0, b2=0.0,
                      eps=0.0, weight_decay=0.0, max_grad_norm=-1)
    want = 0.5 * (1.0 + math.cos(math.pi * 5 / 8))
    assert abs(float(-p[0]) - want) < 1e-7 and bool((p == p[0]).all())


def test_shadows_are_the_exact_casts_of_the_updated_parameters(fx):
    p, _, _, sh, shf, covered = _run_case(fx, "main", shadows=True)
    assert torch.equal(sh[covered], p[covered].to(torch.bfloat16)) and torch.equal(shf[covered], p[covered].to(torch.float16))
    assert bool((sh[~covered].float() == 9.0).all()) and bool((shf[~covered].float() == 9.0).all())


def test_scaler_state_skips_an_overflowed_step_and_drives_the_schedule(fx):
    offs, sizes, decay = fx["offsets"].tolist(), fx["sizes"].tolist(), fx["decay"].tolist()
    tensors, chunks = _dev_tables([(o, s, d, True) for o, s, d in zip(offs, sizes, decay)])
    part, sq = torch.zeros(chunks.numel(), device=DEV), torch.zeros(len(sizes), device=DEV)
    lr, warmup, t_total, b1, b2, e, wd, mgn = [float(x) for x in fx["main/hyper"]]
    kw = dict(lr=lr, warmup=warmup, t_total=int(t_total), schedule="warmup_linear", b1=b1, b2=b2, eps=e, weight_decay=wd, max_grad_norm=mgn)
    p = torch.from_numpy(fx["p0"]).to(DEV).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sh = torch.full_like(p, 9.0).to(torch.bfloat16)
    state = torch.tensor([1024.0, 1 / 1024.0, 0, 1.0, 0, 1, 0, 0], device=DEV)      # skip flag set, no step applied yet
    g = torch.from_numpy(fx["grads"][0]).to(DEV)
    ops.tensor_sqnorms(g, tensors, chunks, part, sq)
    ops.bertadam_step(p, g, m, v, tensors, chunks, sq, step=99, shadow=sh, scaler_state=state, **kw)
    assert torch.equal(p.cpu(), torch.from_numpy(fx["p0"])) and float(m.abs().max()) == 0 and float(v.abs().max()) == 0
    assert bool((sh.float() == 9.0).all())
    # a freshly reset state (skip 0, no update counted): treated as step 0 -- lr_t = 0 under warm-up, never a negative rate
    state[3], state[4] = 0.0, 0.0
    p1, m1, v1 = p.clone(), m.clone(), v.clone()
    ops.bertadam_step(p1, g, m1, v1, tensors, chunks, sq, step=99, scaler_state=state, **kw)
    assert torch.equal(p1, p) and float(m1.abs().max()) > 0
    # applied steps: the schedule's step is state[4] - 1 whatever `step` says, so the fixture's trajectory is reproduced
    for s in range(3):
        state[3], state[4] = 0.0, float(s + 1)                          # what mv_scaler_update leaves after a clean step
        g = torch.from_numpy(fx["grads"][s]).to(DEV)
        ops.tensor_sqnorms(g, tensors, chunks, part, sq)
        ops.bertadam_step(p, g, m, v, tensors, chunks, sq, step=99, scaler_state=state, **kw)
        assert float((p - torch.from_numpy(fx["main/p"][s]).to(DEV)).abs().max()) < TOL


def test_new_entry_points_reject_bad_arguments():
    lib = _lib.load()
    n = 256
    x = torch.zeros(n + 4, device=DEV)
    tensors, chunks = _dev_tables([(0, n, True, True)])
    part, out = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.stream_ptr()
    assert lib.mv_tensor_sqnorms(P(x), n, None, 1, P(chunks), 1, P(part), P(out), st) == -1            # null table
    assert lib.mv_tensor_sqnorms(P(x), n, P(tensors), 0, P(chunks), 1, P(part), P(out), st) == -1       # T <= 0
    assert lib.mv_tensor_sqnorms(P(x), n, P(tensors), 1, P(chunks), 0, P(part), P(out), st) == -1
    assert lib.mv_tensor_sqnorms(P(x[1:]), n, P(tensors), 1, P(chunks), 1, P(part), P(out), st) == -2   # misaligned buffer
    assert lib.mv_tensor_sqnorms(P(x), n + 2, P(tensors), 1, P(chunks), 1, P(part), P(out), st) == -2

    def step(p=x, tens=tensors, T=1, sq=out, sched=0, t_total=-1, sh=None):
        return lib.mv_bertadam_step(P(p), P(x), P(x), P(x), None if sh is None else P(sh), None, n, None if tens is None else P(tens), T,
                                    P(chunks), 1, None if sq is None else P(sq), 1e-3, 0.9, 0.999, 1e-6, 0.01, 1.0, 0, t_total, -1.0, sched,
                                    None, st)
    assert step(tens=None) == -1 and step(T=0) == -1 and step(sq=None) == -1 and step(sched=7) == -1 and step(t_total=0) == -1
    assert step(p=x[1:]) == -2
    assert step(sh=torch.zeros(n + 4, dtype=torch.bfloat16, device=DEV)[1:]) == -2
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and float(out.abs().max()) == 0.0      # no refused call launched anything


# ------------------------------------------------------------------------------------------------ optim.BertAdam over the models
CFG = O.CONFIGS["c1"]
NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


def _cfg_dict(c):
    return dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)


def _groups(model):
    """The reference's grouping (main.py:115-120, finetune.py:382-390)."""
    named = list(model.named_parameters())
    return [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
            {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]


def _torch_bertadam(p, g, m, v, step, decay, lr, warmup, t_total, b1=0.9, b2=0.999, e=1e-6, wd=0.01, mgn=1.0):
    """The update rule of the issue / optimization.py:123-175 on one tensor, in plain torch (warmup_linear)."""
    if mgn > 0:
        g = g * min(1.0, mgn / (float(g.norm()) + 1e-6))
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    u = m / (v.sqrt() + e)
    if decay:
        u = u + wd * p
    x = step / t_total
    lr_t = lr * (x / warmup if x < warmup else max((x - 1.0) / (warmup - 1.0), 0))
    p.add_(-lr_t * u)


def _inputs(b):
    return (b["cls_tok"].to(DEV), b["input_txt"].to(DEV), b["attn_mask"].to(DEV), b["segment"].to(DEV),
            (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))


def _three_steps(model, bert, loss_fn, unreached, head=None):
    """3 steps of optim.BertAdam (reference groups, warm-up crossed) against the transcription applied to snapshots of the same
    Parameters and the same gradients; unreached tensors and the flat buffer's alignment gaps must come out bit-unchanged."""
    lr, warmup, t_total = 1e-3, 0.25, 4
    opt = mv.optim.BertAdam(_groups(model), lr=lr, warmup=warmup, t_total=t_total)
    named = dict(model.named_parameters())
    decay_ids = {id(p) for k, p in named.items() if not any(nd in k for nd in NO_DECAY)}      # from the names, not from the optimizer
    eng = bert.engine
    covered = torch.zeros(eng.n_flat, dtype=torch.bool, device=DEV)
    for off, shape in eng.layout.values():
        covered[off:off + math.prod(shape)] = True
    with torch.no_grad():
        eng.flat_p[~covered] = 3.25
    start = {k: p.detach().clone() for k, p in named.items()}
    ref = {k: p.detach().clone() for k, p in named.items()}
    mom = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in named.items()}
    assert opt.get_lr() == [0]
    for s in range(3):
        opt.zero_grad()
        loss_fn().backward()
        grads = {k: p.grad.detach().clone() for k, p in named.items()}
        opt.step()
        for k, p in named.items():
            if k.startswith(unreached):
                continue
            _torch_bertadam(ref[k], grads[k], *mom[k], s, id(p) in decay_ids, lr, warmup, t_total)
            err = float((p.detach() - ref[k]).abs().max())
            assert err < TOL, (k, s, err)
        if s == 0:                                                      # step 0: lr_t = 0 moves nothing, the moments are updated
            assert all(torch.equal(p.detach(), start[k]) for k, p in named.items())
            assert float(eng.flat_m.abs().max()) > 0
        assert abs(opt.get_lr()[0] - lr * ((s + 1) / t_total / warmup if (s + 1) / t_total < warmup
                                           else (((s + 1) / t_total) - 1) / (warmup - 1))) < 1e-12
    moved = [k for k, p in named.items() if not torch.equal(p.detach(), start[k])]
    assert len(moved) > 10
    for k, p in named.items():
        if k.startswith(unreached):
            assert torch.equal(p.detach(), start[k]), k                # no update and no weight decay
    assert bool((eng.flat_p[~covered] == 3.25).all())
    for sh in (eng.shadow, eng.shadow_f):                               # the 16-bit copies the next forward reads are current
        if sh is not None:
            assert torch.equal(sh[covered], eng.flat_p[covered].to(sh.dtype))
    assert not bert._params_dirty()
    if head is not None:
        assert not head._head_dirty()
        for sh in (head.head_sh, head.head_shf):
            if sh is not None:
                assert torch.equal(sh, head.head_p.to(sh.dtype))
    return opt


def test_bertadam_over_cxrbert_equals_the_transcription():
    P = O.make_params(CFG, seed=3)
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, 4, 16, 45, "full", seed=11).items()}
    m = mv.CXRBERT(_cfg_dict(CFG), None, dtype=torch.bfloat16, device=DEV)
    m.load_state_dict(P)
    m.eval()

    def loss_fn():
        mlm, itm = m(*_inputs(b))
        return mv.losses.mlm_itm_loss(mlm, itm, b["txt_labels"].to(DEV), b["is_aligned"].to(DEV))
    opt = _three_steps(m, m, loss_fn, unreached=("\0",))
    # state dict round trip: a second optimizer continues from the same step and moments
    sd = opt.state_dict()
    assert sd["step"] == 3 and sd["flat_m"].shape == m.engine.flat_p.shape
    opt2 = mv.optim.BertAdam(_groups(m), lr=1.0)
    opt2.load_state_dict(sd)
    assert opt2._t == 3 and opt2.param_groups[0]["lr"] == 1e-3 and opt2.param_groups[0]["t_total"] == 4


def test_bertadam_over_the_vqa_model_leaves_unreached_heads_bit_unchanged():
    P = O.make_params(CFG, seed=3)
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, 4, 16, 45, "s2s", seed=11).items()}
    g = torch.Generator().manual_seed(4)
    target = (torch.rand(4, 458, generator=g) < 0.01).float()
    m = mv.CXRBertForVQA(_cfg_dict(CFG), dtype=torch.bfloat16, device=DEV)
    m.bert.load_state_dict(P, strict=True)
    m.eval()
    opt = _three_steps(m, m.bert, lambda: m(*_inputs(b), ans_labels=target.to(DEV))[1],
                       unreached=("bert.mlm.", "bert.itm.", "bert.enc.pooler."), head=m)
    assert opt._task is m
    pad = m._view(m.head_p, "ans_classifier.2.weight", padded=True)[458:]
    assert float(pad.abs().max()) == 0.0                                # the padding rows of the classifier stay zero


def test_bertadam_over_the_classification_model_updates_the_pooler_and_skips_the_heads():
    """The one task where the pooler is ACTIVE while the MLM and ITM heads are not."""
    P = O.make_params(CFG, seed=3)
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, 4, 16, 45, "1d", seed=11).items()}
    labels = (torch.rand(4, 14, generator=torch.Generator().manual_seed(4)) < 0.3).float()
    m = mv.CXRBertForClassification(_cfg_dict(CFG), dtype=torch.bfloat16, device=DEV, n_classes=14)
    m.bert.load_state_dict(P, strict=True)
    m.eval()
    start = m.bert.get_parameter("enc.pooler.dense.weight").detach().clone()
    opt = _three_steps(m, m.bert, lambda: m(*_inputs(b), labels=labels.to(DEV)), unreached=("bert.mlm.", "bert.itm."), head=m)
    assert opt._task is m
    assert not torch.equal(m.bert.get_parameter("enc.pooler.dense.weight").detach(), start)
    pad = m._view(m.head_p, "clf.weight", padded=True)[14:]
    assert tuple(pad.shape) == (2, CFG.hidden) and float(pad.abs().max()) == 0.0
