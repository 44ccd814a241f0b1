"""The reference's training loop around the drop-in model, in the reference's own step order (train_origin.py:106-131):

    mlm, itm = model(...); loss = ...
    optimizer.zero_grad()
    loss.backward(); optimizer.step()

The loss runs BEFORE zero_grad(), and from the second step on every .grad is a view of the engine's flat gradient buffer when it runs
(CXRBERT.grad_views).  Every backward here is held to autograd's rule (`backward_by_the_rule`): .grad after backward() = what .grad held when
backward() started + this backward's gradient, the latter computed independently -- by the CPU oracle (fp32 loop), or by the same model
run the way the rest of the suite runs it (zero_grad() first, gradients handed over as copies).  Several steps, alternating two batches, so
that a gradient left over from the previous step cannot pass for this one.  Adam is nearly blind to a constant gradient factor, so the
gradients are compared, not only the parameters."""
import pytest
import torch

import medvill_amd as mv
from oracle import cxrbert_oracle as O
from oracle import synth
from tests.test_model_gpu import DEV, fwd, load_case, make_model

pytestmark = pytest.mark.gpu

LR = 1e-3
CASES = ["c1v1k_full", "c1v1k_bar_ragged"]
# CXRBERT(dtype=..., grad_operand=...): the exact path; 16-bit with loss-scaled f16 gradient operands (default); 16-bit with bf16 ones
PRECISIONS = {"fp32": (torch.float32, None), "bf16_f16grad": (torch.bfloat16, None), "bf16_bf16grad": (torch.bfloat16, "bf16")}
# the literal logits + the two CrossEntropyLoss calls; lazy logits + mlm_itm_loss; the same with forward(..., txt_labels=); the same with
# the head's gradient taken in the backward instead of the loss (model.grad_in_loss = False)
PATHS = ["literal", "lazy", "lazy_labels", "lazy_grad_in_backward"]
# zero_grad -> forward -> loss -> backward (what the other tests do); forward -> loss -> zero_grad -> backward (the reference's order)
# with model.zero_grad(), model.zero_grad(set_to_none=False) and optimizer.zero_grad()
ORDERS = ["zero_first", "reference", "reference_keep", "reference_optimizer"]
ORACLE_RTOL, HIP_RTOL, B16_RTOL = 1e-3, 2e-4, 3e-2


def batches(golden_dir, name):
    """The golden case's batch and a second one of the same shape and mask family (another seed)."""
    z, meta, cfg, P, b = load_case(golden_dir, name)
    b2 = synth.make_batch(cfg, meta["B"], meta["N"], meta["S"], meta["family"], seed=meta["seed"] + 1)
    return cfg, P, [b, {k: torch.from_numpy(v) for k, v in b2.items()}]


def build(cfg, P, prec, path, views=None):
    dtype, gop = PRECISIONS[prec]
    model = make_model(cfg, P, dtype, grad_operand=gop)
    model.lazy_logits = path != "literal"
    model.grad_in_loss = path != "lazy_grad_in_backward"
    model.grad_views = views
    return model


def forward(model, b, path):
    if path == "lazy_labels":
        return model(b["cls_tok"].to(DEV), b["input_txt"].to(DEV), b["attn_mask"].to(DEV), b["segment"].to(DEV),
                     (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV), txt_labels=b["txt_labels"].to(DEV))
    return fwd(model, b)


def loss_from(out, b, task):
    """itm_loss + mlm_loss of train_origin.py:108-126 (a task switched off contributes nothing); on plain logits exactly the two torch
    cross-entropies, on a LazyLogits handle the fused head."""
    return mv.losses.mlm_itm_loss(out[0], out[1], b["txt_labels"].to(DEV), b["is_aligned"].to(DEV), **task)


def zero_grad(order, model, opt):
    if order == "reference_keep":
        model.zero_grad(set_to_none=False)
    elif order == "reference_optimizer":
        opt.zero_grad()
    else:
        model.zero_grad()


def grads_of(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def grads_held(model):
    return {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()}


def checked_loss(model, b, path, task=None, out=None):
    """forward (unless its output `out` is given) + loss, which must leave .grad as it was: only backward() and zero_grad() change it."""
    held = grads_held(model)
    if out is None:
        out = forward(model, b, path)
    loss = loss_from(out, b, task or {})
    for n, p in model.named_parameters():
        assert (p.grad is None) == (held[n] is None) and (p.grad is None or torch.equal(p.grad, held[n])), n
    return loss


def backward_by_the_rule(model, loss, this, rtol, **kw):
    """loss.backward(**kw), then autograd's rule for every Parameter: .grad = (what .grad held when backward() started) + `this` (the
    gradient of this backward, computed independently).  Per tensor |got - want| <= rtol * max(max|want|, 1e-3 * the largest |want|)."""
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(this)                   # every Parameter once (tied / aliased tensors are one Parameter)
    before = grads_held(model)
    loss.backward(**kw)
    want = {n: this[n].to(DEV, torch.float32) + (0.0 if before[n] is None else before[n].float()) for n in params}
    gmax = max(float(w.abs().max()) for w in want.values())
    for n, p in params.items():
        assert p.grad is not None, n
        err = float((p.grad.detach().float() - want[n]).abs().max())
        scale = max(float(want[n].abs().max()), 1e-3 * gmax)
        assert err <= rtol * scale, (n, err, scale)


def run_loop(golden_dir, name, prec, path, order, views=None, task=None, steps=3, twin_path=None):
    """`steps` optimizer steps of medvill_amd.optim.AdamW, batches alternating.  Reference: the oracle's loop body (autograd + HF AdamW,
    oracle.cxrbert_oracle.train_step) for the exact path with both tasks; otherwise a twin model (path `twin_path`, default the same) run with
    zero_grad() first and gradients handed over as copies, stepped by its own optimizer."""
    task = task or {}
    cfg, P, bs = batches(golden_dir, name)
    model = build(cfg, P, prec, path, views)
    opt = mv.optim.AdamW(model.parameters(), lr=LR)
    oracle = prec == "fp32" and not task
    if oracle:
        Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        Mo = {k: torch.zeros_like(v) for k, v in P.items()}
        Vo = {k: torch.zeros_like(v) for k, v in P.items()}
        rtol = ORACLE_RTOL
    else:
        twin = build(cfg, P, prec, twin_path or path, views=False)
        topt = mv.optim.AdamW(twin.parameters(), lr=LR)
        rtol = HIP_RTOL if prec == "fp32" else B16_RTOL
    for t in range(1, steps + 1):
        b = bs[(t - 1) % 2]
        if oracle:
            O.train_step(Po, Mo, Vo, t, cfg, b, lr=LR, training=False)        # leaves this step's gradient in Po[k].grad
            this = {k: w.grad for k, w in Po.items()}
            after = {k: w.detach() for k, w in Po.items()}
        else:
            twin.zero_grad()
            loss_from(forward(twin, b, twin_path or path), b, task).backward()
            this = grads_of(twin)
            topt.step()
            after = {n: p.detach() for n, p in twin.named_parameters()}
        if order == "zero_first":
            zero_grad(order, model, opt)
        loss = checked_loss(model, b, path, task)
        if path != "literal" and prec != "fp32" and name == "c1v1k_full":
            assert model.engine.S["cu"] is not None              # the Dataset's matrix was recognised: packed rows, as by default
        if order != "zero_first":
            zero_grad(order, model, opt)
        backward_by_the_rule(model, loss, this, rtol)
        opt.step()
        for n, p in model.named_parameters():
            d = (p.detach() - after[n].to(DEV)).abs()
            if oracle:
                assert float(d.max()) < 2e-4, (t, n, float(d.max()))     # as test_train_steps_follow_the_oracle: fp32 rounding only
            else:
                # two runs of a 16-bit path (or of the fp32 atomics) differ in the low bits of every gradient, and Adam turns a gradient
                # that is nothing but those bits into a step of up to ~lr
                assert float(d.max()) <= 6 * LR * t and float((d > 0.1 * LR).float().mean()) < 5e-2, (t, n, float(d.max()))


# ------------------------------------------------------------------------------------------------ (a) the loop, step by step
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("name", CASES)
def test_every_step_of_the_loop_has_that_steps_gradient(golden_dir, name, prec, path, order):
    run_loop(golden_dir, name, prec, path, order)


@pytest.mark.parametrize("views", [None, True, False])
@pytest.mark.parametrize("order", ["reference", "reference_keep"])
@pytest.mark.parametrize("path", PATHS[1:])
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_reference_order_with_gradient_views_and_copies(golden_dir, prec, path, order, views):
    """model.grad_views: views of the flat buffer (None = automatic, True) are what a loss computed before zero_grad() meets; the copies
    (False) must stay right as well."""
    run_loop(golden_dir, "c1v1k_full", prec, path, order, views=views)


# ------------------------------------------------------------------------------------------------ (b) accumulation in the reference order
ACCUMULATION = ["two_micro_batches", "half_loss_after_zeroing_in_place", "retain_graph", "loss_never_backpropagated",
                "two_losses_on_one_handle"]


def accumulation_setup(golden_dir, prec, path):
    """The model under test with a previous step's gradient of batch B in .grad (what the reference's loop meets from step 2 on), and the
    single-step gradients of batches A and B from the literal path after zero_grad() (copies, never views)."""
    cfg, P, (bA, bB) = batches(golden_dir, "c1v1k_full")
    twin = build(cfg, P, prec, "literal", views=False)
    g = []
    for b in (bA, bB):
        twin.zero_grad()
        loss_from(forward(twin, b, "literal"), b, {}).backward()
        g.append(grads_of(twin))
    model = build(cfg, P, prec, path)
    rtol = HIP_RTOL if prec == "fp32" else B16_RTOL
    model.zero_grad()
    backward_by_the_rule(model, checked_loss(model, bB, path), g[1], rtol)
    return model, bA, bB, g[0], g[1], rtol


@pytest.mark.parametrize("case", ACCUMULATION)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", ["fp32", "bf16_f16grad"])
def test_accumulation_follows_autograds_rule_in_the_reference_order(golden_dir, prec, path, case):
    model, bA, bB, gA, gB, rtol = accumulation_setup(golden_dir, prec, path)
    if case == "two_micro_batches":
        # no zero_grad between two micro-batches: gA + gB, each its own mean (not the gradient of the concatenated batch)
        loss = checked_loss(model, bA, path)
        model.zero_grad()
        backward_by_the_rule(model, loss, gA, rtol)
        backward_by_the_rule(model, checked_loss(model, bB, path), gB, rtol)
    elif case == "half_loss_after_zeroing_in_place":
        loss = checked_loss(model, bA, path)
        model.zero_grad(set_to_none=False)
        backward_by_the_rule(model, 0.5 * loss, {n: 0.5 * v for n, v in gA.items()}, rtol)
    elif case == "retain_graph":
        loss = checked_loss(model, bA, path)
        model.zero_grad()
        backward_by_the_rule(model, loss, gA, rtol, retain_graph=True)
        backward_by_the_rule(model, loss, gA, rtol)                     # 2 gA
    elif case == "loss_never_backpropagated":
        checked_loss(model, bA, path)                    # grad enabled, never back-propagated
        loss = checked_loss(model, bB, path)
        model.zero_grad()
        backward_by_the_rule(model, loss, gB, rtol)
    elif case == "two_losses_on_one_handle":
        out = forward(model, bA, path)
        checked_loss(model, bA, path, out=out)
        backward_by_the_rule(model, checked_loss(model, bA, path, out=out), gA, rtol)   # no zero_grad: gB held + gA
    else:
        raise AssertionError(case)


@pytest.mark.parametrize("path", PATHS)
def test_loss_scale_retry_in_the_reference_order(golden_dir, path):
    """f16 gradient operands with a loss scale far past f16's range: the backward overflows, redoes itself with a smaller scale and hands
    over one step's gradient -- with the loss computed before zero_grad() and the views of the previous step in .grad."""
    model, bA, bB, gA, gB, rtol = accumulation_setup(golden_dir, "bf16_f16grad", path)
    out = forward(model, bA, path)
    model.engine.reset_scaler(2.0 ** 40)
    loss = checked_loss(model, bA, path, out=out)
    model.zero_grad()
    backward_by_the_rule(model, loss, gA, rtol)
    assert float(model.engine.scaler[0]) < 2.0 ** 40                    # the retry did happen


@pytest.mark.parametrize("task", [{"mlm_task": False}, {"itm_task": False}], ids=["itm_only", "mlm_only"])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", ["fp32", "bf16_f16grad"])
def test_one_task_switched_off_in_the_reference_order(golden_dir, prec, path, task):
    """train_origin.py:108-116: mlm_task / itm_task off, two steps in the reference's order, against the literal path with that task off."""
    run_loop(golden_dir, "c1v1k_full", prec, path, "reference", task=task, steps=2, twin_path="literal")


# ------------------------------------------------------------------------------------------------ (c) VQA in its reference order
@pytest.mark.parametrize("dtype,rtol", [(torch.float32, HIP_RTOL), (torch.bfloat16, B16_RTOL)])
def test_vqa_loop_in_the_reference_order(dtype, rtol):
    """The VQA fine-tuning loop's order (finetune.py:443-451: backward, step, zero_grad) over 3 steps on two batches: every .grad of the
    encoder and of the answer classifier equals a twin's that hands its gradients over as copies."""
    from tests.test_vqa_gpu import CFG, _batch, _inputs, _model
    P = O.make_params(CFG, seed=3)
    bs = [_batch("s2s", seed=11), _batch("s2s", seed=12)]
    model, twin = _model(dtype, P), _model(dtype, P)
    twin.bert.grad_views = False
    lr = 1e-4
    opt, topt = mv.optim.AdamW(model.parameters(), lr=lr), mv.optim.AdamW(twin.parameters(), lr=lr)
    for t in range(3):
        b = bs[t % 2]
        _, tl = twin(*_inputs(b), ans_labels=b["target"].to(DEV), ans_type=b["ans_type"].to(DEV))
        tl.backward()
        this = grads_of(twin)
        topt.step()
        topt.zero_grad()
        _, loss = model(*_inputs(b), ans_labels=b["target"].to(DEV), ans_type=b["ans_type"].to(DEV))
        backward_by_the_rule(model, loss, this, rtol)
        opt.step()
        opt.zero_grad()
