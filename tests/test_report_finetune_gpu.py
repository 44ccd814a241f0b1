"""Report-generation fine-tuning on the MI355X: the kernels of csrc/mv_lmloss.hip against the fp64 restatement of the reference's
objective (tests/report_finetune_cases.py), and CXRBertForReportFinetune against the oracle encoder (oracle/cxrbert_oracle.py, CPU
autograd) + that restatement.

Tolerances.  Kernels: the project's own, from test_vqa_gpu.py::test_bce_fwd_bwd_matches_torch -- loss and per-entry loss 1e-5 relative,
gradient 1e-6 / 2e-2 / 3e-3 (f32 / bf16 / f16) times the total scale (here 0.5 * 4): a gradient entry is w (Q softmax - q) / (kept
weight sum + 1e-5), at most 1 in magnitude before scaling, like sigmoid - y there.  Model: those of test_vqa_gpu.py's model-level
tests for the same dtype (loss 1e-4 / 1e-2, gradients 2e-4 / 3e-2 by _compare_grads' norm-relative measure with its floor).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                     # noqa: E402
from medvill_amd import hip_ops as ops       # noqa: E402
from medvill_amd import losses               # noqa: E402
from oracle import cxrbert_oracle as O       # noqa: E402
from oracle import synth                     # noqa: E402
import report_finetune_cases as C            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GTOL = {torch.float32: 1e-6, torch.bfloat16: 2e-2, torch.float16: 3e-3}
UPSTREAM, LOSS_SCALE = 0.5, 4.0


# ------------------------------------------------------------------------------------------------ kernels
def _run_kernels(case, ls, ratio, gdt):
    d = {k: case[k].to(DEV) for k in ("logits", "row_ptr", "labels", "weights", "sample")}
    B, V, ld, U = case["B"], case["V"], case["ld"], case["U"]
    k = C.keep_count(B, ratio)
    loss_e, hit, row_stat = ops.lm_loss_fwd(d["logits"], d["row_ptr"], d["labels"], ls, U=U, V=V, ld=ld)
    keep, stats, inv = ops.lm_loss_select(loss_e, d["weights"], d["sample"], hit, B, k)
    dl = torch.full((U, ld), 7.0, device=DEV).to(gdt)
    g = torch.tensor([UPSTREAM], device=DEV)
    S = torch.tensor([LOSS_SCALE], device=DEV)
    ops.lm_loss_bwd(d["logits"], d["row_ptr"], d["labels"], d["weights"], d["sample"], ls, row_stat, keep, inv, g, dl, U=U, V=V, ld=ld,
                    ldd=ld, loss_scale_dev=S)
    torch.cuda.synchronize()
    return dict(loss_e=loss_e.cpu(), hit=hit.cpu(), keep=keep.cpu(), stats=stats.cpu(), dl=dl.cpu(), k=k)


def _check(case, ls, ratio, gdt):
    got = _run_kernels(case, ls, ratio, gdt)
    ref = C.reference(case, ls, ratio, scale=UPSTREAM * LOSS_SCALE)
    V = case["V"]
    el, rl = got["loss_e"].double(), ref["entry_loss"]
    rel = ((el - rl).abs() / rl.abs().clamp(min=1e-300)).where(rl != 0, (el != 0).double())
    gerr = float((got["dl"][:, :V].double() - ref["grad"]).abs().max()) if case["U"] else 0.0
    lerr = abs(float(got["stats"][0]) - ref["loss"])
    print(f"V={V} B={case['B']} ls={ls} ratio={ratio} {gdt}: entry rel {float(rel.max()) if rel.numel() else 0.0:.2e} "
          f"loss {float(got['stats'][0]):.7f} ref {ref['loss']:.7f} grad err {gerr:.2e}")
    assert torch.isfinite(el).all() and torch.isfinite(got["stats"]).all()
    assert float(rel.max()) < 1e-5 if rel.numel() else True
    assert lerr <= 1e-5 * abs(ref["loss"])
    assert torch.equal(got["keep"].bool(), ref["keep"])
    w_kept = float(case["slot_weights"][ref["keep"]].sum())
    assert abs(float(got["stats"][1]) - w_kept) < 1e-6 and float(got["stats"][2]) == float(got["k"])
    assert gerr < GTOL[gdt] * UPSTREAM * LOSS_SCALE
    if case["U"]:
        assert float(got["dl"][:, V:].float().abs().max()) == 0.0               # pad columns written as zero
        # rows without a kept entry of positive weight and mass: exactly zero
        zero = ref["grad"].abs().amax(dim=1) == 0
        assert float(got["dl"][zero].float().abs().max() if bool(zero.any()) else 0.0) == 0.0
    # argmax hits: entries of kept samples with a positive weight
    am = case["logits"][:, :V].argmax(1) if case["U"] else torch.zeros(0, dtype=torch.int64)
    rows = torch.repeat_interleave(torch.arange(case["U"]), (case["row_ptr"][1:] - case["row_ptr"][:-1]).long())
    hits = sum(1 for e in range(case["n"]) if bool(ref["keep"][int(case["sample"][e])]) and float(case["weights"][e]) > 0
               and int(am[rows[e]]) == int(case["labels"][e]))
    assert float(got["stats"][3]) == float(hits)
    return got


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,ratio", [(5, 0.0), (5, 0.2), (1, 0.2), (10, 0.9)])
@pytest.mark.parametrize("ls", [0.0, 0.1, 1.0])
def test_kernels_match_the_restatement_small_vocabulary(ls, B, ratio, gdt):
    _check(C.make_case(B, 300, 304, seed=3 + B), ls, ratio, gdt)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ratio", [0.0, 0.2])
@pytest.mark.parametrize("ls", [0.0, 0.1, 1.0])
def test_kernels_match_the_restatement_bert_vocabulary(ls, ratio, gdt):
    case = C.make_case(5, 30522, 30528, seed=8, extra=False)
    assert case["U"] == 5
    _check(case, ls, ratio, gdt)


def test_unaligned_leading_dimension_takes_the_scalar_path():
    case = C.make_case(5, 300, 301, seed=5)
    _check(case, 0.1, 0.2, torch.float32)


def test_saturated_and_all_equal_rows():
    case = C.make_case(5, 300, 304, seed=3)
    got = _run_kernels(case, 0.0, 0.0, torch.float32)
    lab = case["labels"].tolist()
    sat = [e for e in range(case["n"]) if int(case["sample"][e]) == 4 and lab[e] == 3][0]
    eq = [e for e in range(case["n"]) if int(case["sample"][e]) == 4 and lab[e] == 4][0]
    import math
    assert abs(float(got["loss_e"][sat]) - math.log(40.0)) < 1e-5 * math.log(40.0)         # 40 columns at +80, 260 at -80
    assert abs(float(got["loss_e"][eq]) - math.log(300.0)) < 1e-5 * math.log(300.0)
    assert int(got["hit"][sat]) == 0 and int(got["hit"][eq]) == 0                            # argmax is column 0 (first maximum)


def test_two_runs_give_bitwise_equal_results():
    case = C.make_case(10, 300, 304, seed=13)
    a, b = _run_kernels(case, 0.1, 0.2, torch.float32), _run_kernels(case, 0.1, 0.2, torch.float32)
    assert a["stats"].view(torch.int32).tolist() == b["stats"].view(torch.int32).tolist()
    assert torch.equal(a["loss_e"].view(torch.int32), b["loss_e"].view(torch.int32)) and torch.equal(a["dl"], b["dl"])


def test_tie_between_identical_samples_goes_to_the_lower_index():
    case = C.make_case(2, 300, 304, seed=17, identical=True)
    got = _run_kernels(case, 0.1, 0.5, torch.float32)                  # k = 1
    assert got["keep"].tolist() == [1, 0]
    ref = C.reference(case, 0.1, 0.5)                                  # the value does not depend on the choice
    assert abs(float(got["stats"][0]) - ref["loss"]) <= 1e-5 * ref["loss"]


# ------------------------------------------------------------------------------------------------ model against the oracle
CFG = O.CONFIGS["c1"]
N_REG, S_TXT, BATCH, MAX_PRED = 16, 45, 4, 4
LTOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2, torch.float16: 1e-2}
RTOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2, torch.float16: 3e-2}
UNREACHED = ("itm.", "enc.pooler.")


def _cfg_dict(c):
    return dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)


def _batch(family, seed=11, plain=False):
    """synth batch + the listed predictions: sample 0 lists its last [SEP] twice, sample 1 has two padded slots, sample 2 a label 0.
    `plain`: all weights 1, no duplicates (the existing lazy route can express it)."""
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, BATCH, N_REG, S_TXT, family, seed=seed).items()}
    g = torch.Generator().manual_seed(seed)
    pos = torch.zeros(BATCH, MAX_PRED, dtype=torch.int64)
    lab = torch.zeros(BATCH, MAX_PRED, dtype=torch.int64)
    w = torch.zeros(BATCH, MAX_PRED)
    for s in range(BATCH):
        n = int(b["n_ids"][s])                                        # text ids including the last [SEP]
        picks = (torch.randperm(n - 1, generator=g)[:MAX_PRED] + N_REG + 2).tolist()
        last = N_REG + 2 + n - 1
        if s == 0 and not plain:
            picks = [picks[0], last, picks[1], last]
        pos[s] = torch.tensor(picks)
        lab[s] = torch.randint(1, CFG.vocab_size, (MAX_PRED,), generator=g)
        w[s] = 1.0
        if s == 0 and not plain:
            lab[s, 1] = lab[s, 3] = 102                                # [SEP]
        if s == 1 and not plain:
            pos[s, 2:], lab[s, 2:], w[s, 2:] = 0, 0, 0.0
        if s == 2 and not plain:
            lab[s, 0], w[s, 1] = 0, 0.5
    b["masked_pos"], b["masked_lm_labels"], b["masked_weights"] = pos, lab, w
    return b


def _model(dtype, P, ls, **kw):
    """torch.float32: the exact path; torch.float16: the 16-bit path with f16 operands (the engine's default); torch.bfloat16: the
    16-bit path with bf16 forward and gradient operands."""
    if dtype == torch.bfloat16:
        kw = dict(fwd_operand="bf16", grad_operand="bf16", **kw)
    m = mv.CXRBertForReportFinetune(_cfg_dict(CFG), dtype=torch.float32 if dtype == torch.float32 else torch.bfloat16, device=DEV,
                                    label_smoothing=ls, **kw)
    m.bert.load_state_dict(P, strict=True)
    m.eval()
    return m


def _inputs(b, mask=None):
    return (b["cls_tok"].to(DEV), b["input_txt"].to(DEV), b["attn_mask"].to(DEV) if mask is None else mask, b["segment"].to(DEV),
            (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))


def _lists(b):
    return dict(masked_lm_labels=b["masked_lm_labels"], masked_pos=b["masked_pos"], masked_weights=b["masked_weights"])


_REF = {}


def _reference(P, b, ls, ratio, key):
    """oracle encoder (CPU, f32 autograd) + transform + tied decoder on the listed rows (model.py:1043-1045) + the restatement."""
    if key in _REF:
        return _REF[key]
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x, _ = O.encode(Pg, CFG, b["cls_tok"], b["input_txt"], b["attn_mask"], b["segment"], b["img_feats"], b["img_pos"], b["sep_tok"])
    rows = torch.gather(x, 1, b["masked_pos"].unsqueeze(2).expand(-1, -1, x.shape[-1]))
    t = O.mlm_transform(Pg, CFG, rows)
    z = torch.nn.functional.linear(t, Pg["enc.txt_embeddings.word_embeddings.weight"]) + Pg["mlm.predictions.bias"]
    loss, keep, _ = C.objective(z, b["masked_lm_labels"], b["masked_weights"], ls, ratio)
    loss.backward()
    _REF[key] = (float(loss.detach()), {k: p.grad for k, p in Pg.items() if p.grad is not None}, keep)
    return _REF[key]


def _compare_grads(got, ref, rtol):
    gmax = max(float(g.abs().max()) for g in ref.values())
    floor = (1e-5 if rtol < 1e-3 else 3e-2) * gmax
    worst = 0.0
    for k, r in ref.items():
        g = got[k].float().cpu()
        n = r.double().norm()
        e1 = float((g.double() - r.double()).norm()) / max(float(n), floor * r.numel() ** 0.5)
        worst = max(worst, e1)
        assert e1 < rtol, (k, e1, float(n))
    return worst


def _mask_of(b, family, how):
    if how == "dense":
        return None
    return mv.data.MaskDesc.make(family, N_REG, S_TXT, b["n_ids"], DEV)


@pytest.mark.parametrize("family", ["s2s", "1d", "bar"])
@pytest.mark.parametrize("dtype,how", [(torch.float32, "dense"), (torch.bfloat16, "dense"), (torch.bfloat16, "desc"),
                                       (torch.float16, "dense"), (torch.float16, "desc")])
@pytest.mark.parametrize("ls,ratio", [(0.1, 0.0), (0.0, 0.25)])
def test_loss_and_every_reached_gradient_match_the_oracle(family, dtype, how, ls, ratio):
    P = O.make_params(CFG, seed=3)
    b = _batch(family)
    m = _model(dtype, P, ls)
    loss, dummy = m(*_inputs(b, _mask_of(b, family, how)), **_lists(b), drop_worst_ratio=ratio)
    loss.backward()
    ref_loss, ref_g, ref_keep = _reference(P, b, ls, ratio, (family, ls, ratio))
    got = {k: p.grad for k, p in m.bert.named_parameters()}
    print(f"{family} {dtype} {how} ls={ls} ratio={ratio}: loss {float(loss):.6f} ref {ref_loss:.6f}")
    assert tuple(dummy.shape) == (1,) and float(dummy) == 0.0
    assert abs(float(loss.detach()) - ref_loss) < LTOL[dtype], (float(loss.detach()), ref_loss)
    if dtype == torch.float32:
        assert torch.equal(m.lm_keep.cpu().bool(), ref_keep)
    assert set(ref_g) <= set(got) and not any(k.startswith(UNREACHED) for k in ref_g) and len(ref_g) > 30
    worst = _compare_grads(got, ref_g, RTOL[dtype])
    print(f"   worst gradient error {worst:.2e}")
    for k, p in m.bert.named_parameters():
        if k.startswith(UNREACHED):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    st = m.lm_stats.cpu()
    assert float(st[0]) == float(loss) and float(st[2]) == float(C.keep_count(BATCH, ratio))


def test_loss_equals_the_lazy_route_without_smoothing_weights_or_duplicates():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s", plain=True)
    m = _model(torch.float32, P, 0.0)
    with torch.no_grad():
        loss, _ = m(*_inputs(b), **_lists(b), drop_worst_ratio=0.0)
    assert m.bert.engine.S["keep"] is False and loss.grad_fn is None          # evaluation keeps no activations
    bert = m.bert
    bert.lazy_logits = True
    L = N_REG + S_TXT + 3
    labels = torch.full((BATCH, L), -100, dtype=torch.int64)
    labels.scatter_(1, b["masked_pos"], b["masked_lm_labels"])
    with torch.no_grad():
        mlm, itm = bert(*_inputs(b))
        lazy = losses.mlm_itm_loss(mlm, itm, labels.to(DEV), b["is_aligned"].to(DEV), itm_task=False)
    # the lazy route is a mean over the 16 labelled rows; this one divides by 16 + 1e-5
    want = float(lazy) * 16.0 / (16.0 + 1e-5)
    assert abs(float(loss) - want) < 1e-5 * want, (float(loss), want)


def test_refused_inputs_and_missing_arguments():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    m = _model(torch.bfloat16, P, 0.1)
    with pytest.raises(ValueError):
        m(*_inputs(b))
    bad = _lists(b)
    bad["masked_pos"] = b["masked_pos"].clone()
    bad["masked_pos"][3, 0] = 0
    with pytest.raises(ValueError, match="position 0"):
        m(*_inputs(b), **bad)
    desc = mv.data.MaskDesc.make("s2s", N_REG, S_TXT, b["n_ids"], DEV)
    bad["masked_pos"][3, 0] = N_REG + 2 + int(b["n_ids"][3])              # the first padded position
    with pytest.raises(ValueError, match="valid length"):
        m(*_inputs(b, desc), **bad)
    bad = _lists(b)
    bad["masked_lm_labels"] = b["masked_lm_labels"].clone()
    bad["masked_lm_labels"][0, 0] = CFG.vocab_size
    with pytest.raises(ValueError, match="vocabulary"):
        m(*_inputs(b), **bad)
    # device tensors are read back once and give the same loss as host tensors
    with torch.no_grad():
        l1, _ = m(*_inputs(b), **_lists(b))
        l2, _ = m(*_inputs(b), **{k: v.to(DEV) for k, v in _lists(b).items()})
    assert float(l1) == float(l2)


def _train(m, b, steps, generate_first=False):
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    out = []
    for i in range(steps):
        if generate_first and i == 1:
            m.generate(b["cls_tok"].to(DEV), (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV), max_len=6)
        opt.zero_grad()
        loss, _ = m(*_inputs(b), **_lists(b), drop_worst_ratio=0.0)
        loss.backward()
        opt.step()
        out.append((float(loss), dict(m.bert.engine.S["drop_keys"]), m.bert.engine.drop_counter))
    return out


def test_three_bertadam_steps_leave_the_unreached_tensors_alone_and_lower_the_loss():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    torch.manual_seed(0)
    m = _model(torch.bfloat16, P, 0.1)
    before = {k: p.detach().clone() for k, p in m.bert.named_parameters()}
    _train(m, b, 3)
    moved = 0
    for k, p in m.bert.named_parameters():
        if k.startswith(UNREACHED):
            assert torch.equal(p.detach(), before[k]), k
        else:
            moved += int(not torch.equal(p.detach(), before[k]))
    assert moved > 10
    m.eval()
    with torch.no_grad():
        after, _ = m(*_inputs(b), **_lists(b))
        m0 = _model(torch.bfloat16, P, 0.1)
        first, _ = m0(*_inputs(b), **_lists(b))
    assert float(after) < float(first), (float(after), float(first))


def test_a_step_after_generate_draws_the_same_dropout_masks():
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    runs = []
    for gen in (False, True):
        torch.manual_seed(0)
        m = _model(torch.bfloat16, P, 0.1)
        runs.append(_train(m, b, 2, generate_first=gen))
    # the same dropout keys and forward count at every step (what generation guarantees); the first step's loss is bitwise equal, the
    # second follows parameters whose gradients went through the embedding backward's f32 atomics
    for (l0, k0, c0), (l1, k1, c1) in zip(*runs):
        assert k0 == k1 and c0 == c1
    assert runs[0][0][0] == runs[1][0][0] and abs(runs[0][1][0] - runs[1][1][0]) < 1e-3 * abs(runs[0][1][0])


def test_finetune_save_and_decode_round_trip(tmp_path):
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    torch.manual_seed(0)
    m = _model(torch.bfloat16, P, 0.1)
    _train(m, b, 2)
    m.eval()
    m.save_pretrained(str(tmp_path))
    gen = mv.CXRBertForGeneration.from_pretrained(str(tmp_path), dtype=torch.bfloat16, device=DEV)
    for k, v in m.bert.state_dict().items():
        assert torch.equal(v.cpu(), gen.bert.state_dict()[k].cpu()), k
    args = (b["cls_tok"].to(DEV), (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))
    ids_a, _ = m.bert.generate(*args, max_len=8)
    ids_b, _ = gen.generate(*args, max_len=8)
    assert torch.equal(ids_a, ids_b)


def test_overflowed_backward_is_redone_with_a_smaller_scale():
    """f16 gradient operands under a loss scale far past f16's range: the backward overflows, redoes itself with S / 16 until everything
    is finite and hands over the gradients of a twin run at the default scale."""
    P = O.make_params(CFG, seed=3)
    b = _batch("s2s")
    grads = []
    for scale in (2.0 ** 40, None):
        m = _model(torch.float16, P, 0.1)
        eng = m.bert.engine
        assert eng.scaler is not None
        loss, _ = m(*_inputs(b), **_lists(b), drop_worst_ratio=0.0)
        if scale is not None:
            eng.reset_scaler(scale)
        loss.backward()
        if scale is not None:
            assert float(eng.scaler[0]) < scale                      # the redo did happen
        grads.append({k: (None if p.grad is None else p.grad.detach().float().cpu()) for k, p in m.bert.named_parameters()})
    got, twin = grads
    for k, g in got.items():
        if k.startswith(UNREACHED):                                   # as the oracle test
            assert g is None or float(g.abs().max()) == 0.0, k
        else:
            assert bool(torch.isfinite(g).all()), k
    _compare_grads(got, {k: g for k, g in twin.items() if not k.startswith(UNREACHED)}, RTOL[torch.float16])
