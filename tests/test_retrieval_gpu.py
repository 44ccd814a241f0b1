"""Retrieval on the MI355X: the three kernels of csrc/mv_retrieval.hip against the numpy definitions of tests/retrieval_cases.py, and
CXRBertForRetrieval.forward(labels=) / fit_step / evaluate / save_pretrained against the oracle encoder (oracle/cxrbert_oracle.py, CPU
autograd) + torch's CrossEntropyLoss, with the tolerances tests/test_classification_gpu.py applies to the same quantities on C1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import medvill_amd as mv
from medvill_amd import hip_ops as ops
from medvill_amd import retrieval as R
from medvill_amd.data import MaskDesc, RetrievalBank
from oracle import cxrbert_oracle as O
from oracle import synth

import retrieval_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = O.CONFIGS["c1"]
N_REG, S_TXT = 16, 45
RANK_CASES = RC.rank_cases()
SAMPLER_CASES = RC.sampler_cases()


# ------------------------------------------------------------------------------------------------ mv_rank_groups
@pytest.mark.parametrize("name", sorted(RANK_CASES))
def test_rank_groups_equals_the_definition_on_its_own_p(name):
    c = RANK_CASES[name]
    C, G = c["C"], c["G"]
    logits, labels = torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)
    p, pos, rank, cnt = ops.rank_groups(logits, labels, C, RC.KS)
    ops.rank_groups(logits, labels, C, RC.KS, counters=cnt)                       # a second launch accumulates
    ph, posh, rankh, cnth = p.cpu().numpy(), pos.cpu().numpy(), rank.cpu().numpy(), cnt.cpu().tolist()
    want_p = torch.softmax(torch.from_numpy(c["logits"]), dim=-1)[:, 1].numpy()
    nan = np.isnan(want_p)
    err = float(np.abs(ph[~nan] - want_p[~nan]).max()) if (~nan).any() else 0.0
    print(f"rank {name}: G={G} C={C} max |p - softmax| = {err:.2e}")
    assert np.array_equal(np.isnan(ph), nan) and err <= 1e-6 and (ph[~nan] >= 0).all() and (ph[~nan] <= 1).all()
    want_pos = RC.positions(ph, C)                                                # the order of the p the kernel WROTE
    assert np.array_equal(posh, want_pos)
    assert np.array_equal(rankh, RC.group_ranks(want_pos, c["labels"], C))
    assert cnth == [2 * v for v in RC.counters(want_pos, c["labels"], C)]
    if name.startswith("saturated"):
        assert int((ph == 1.0).sum()) > C                                         # many exact ties at 1.0: the tie rule decides
    if name.startswith("nan"):
        g1 = slice(C, 2 * C)
        assert int(nan.sum()) == 1 and posh[g1][nan[g1]].tolist() == [C - 1]      # NaN sorts last


def test_rank_counters_feed_summarize():
    c = RANK_CASES["C7_G3"]
    _, pos, _, cnt = ops.rank_groups(torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV), 7, (1, 2, 3, 4, 5, 6, 7, 8))
    s = R.summarize(cnt.cpu().tolist(), (1, 2, 3, 4, 5, 6, 7, 8))                  # 8 cut-offs, one beyond C
    assert s["groups"] == 3 and s["recall"]["R@7"] == 1.0 and s["recall"]["R@8"] == 1.0 and s["hits"]["R@7"] == 1.0
    assert s["precision"]["R@8"] == float((c["labels"] == 1).sum()) / (8 * 3)


# ------------------------------------------------------------------------------------------------ mv_pair_negatives
@pytest.mark.parametrize("name", sorted(SAMPLER_CASES))
def test_pair_negatives_on_shared_draws(name):
    c = SAMPLER_CASES[name]
    idx = torch.tensor(c["idx"], dtype=torch.int32, device=DEV)
    cls = None if c["class_id"] is None else torch.from_numpy(c["class_id"]).to(DEV)
    pairs, labels = ops.pair_negatives(idx, c["n"], class_id=cls, draws=torch.from_numpy(c["draws"].astype(np.int64)))
    wp, wl = RC.sample_negatives(c["idx"], c["n"], c["draws"], c["class_id"])
    assert pairs.cpu().numpy().tolist() == wp.tolist() and labels.cpu().numpy().tolist() == wl.tolist()


@pytest.mark.parametrize("n,classes", [(2, False), (3, True), (1000, False), (1000, True)])
def test_pair_negatives_on_hash_draws_read_back(n, classes):
    rng = np.random.default_rng(n)
    B = 300                                                                       # more than one block
    idx_h = np.concatenate([[0, n - 1], rng.integers(0, n, B - 2)]).astype(np.int32)
    cls_h = rng.integers(0, 2, n).astype(np.int32) if classes else None
    idx = torch.from_numpy(idx_h).to(DEV)
    cls = None if cls_h is None else torch.from_numpy(cls_h).to(DEV)
    pairs, labels = ops.pair_negatives(idx, n, key=0xC0FFEE1234, step=7, class_id=cls)
    draws = ops.pair_draws(0xC0FFEE1234, 7, B, RC.MAX_DRAWS, DEV).cpu().numpy().astype(np.uint64)
    wp, wl = RC.sample_negatives(idx_h, n, draws, cls_h)
    assert pairs.cpu().numpy().tolist() == wp.tolist() and labels.cpu().numpy().tolist() == wl.tolist()
    other, _ = ops.pair_negatives(idx, n, key=0xC0FFEE1234, step=8, class_id=cls)
    assert n == 2 or not torch.equal(other, pairs)                                # another step, another stream
    assert torch.equal(ops.pair_negatives(idx, n, key=0xC0FFEE1234, step=7, class_id=cls)[0], pairs)
    d = draws[:, 0, :].astype(np.float64)
    assert 0.4 < float((d[:, 1] >= 2 ** 31).mean()) < 0.6 and 0.4 < float(d[:, 0].mean() / 2 ** 32) < 0.6


# ------------------------------------------------------------------------------------------------ mv_pair_assemble
@pytest.mark.parametrize("shape", RC.PAIR_SHAPES)
@pytest.mark.parametrize("dtype", [{"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[n] for n in RC.PAIR_DTYPES])
def test_pair_assemble_is_bit_exact(shape, dtype):
    assert RC.PAIR_SHAPES[1] == (N_REG, S_TXT, CFG.img_hidden)                    # the shape of the model tests below
    N, S, Fd = shape
    ids, lens, feats, pos = RC.make_banks(9, 7, N, S, Fd, seed=N + S)
    ft = torch.from_numpy(feats).to(dtype)
    bank = RetrievalBank(None, device=DEV, feat_dtype=dtype)
    bank.add_texts(ids, lens).add_images((ft, torch.from_numpy(pos)))
    pairs = [(0, 0), (6, 8), (3, 0), (3, 0), (2, 8), (6, 1), (0, 5)]               # lengths 1 and S+1, the same item twice, both bank ends
    want = RC.assemble(ids, lens, ft.float().numpy(), pos, pairs)
    for given in (pairs, torch.tensor(pairs, dtype=torch.int32, device=DEV)):     # host list (checked there) / device tensor
        cls_tok, txt, desc, seg, (f, p_), sep_tok = bank.assemble(given)
        assert np.array_equal(txt.cpu().numpy(), want["input_txt"]) and np.array_equal(seg.cpu().numpy(), want["segment"])
        assert f.dtype == dtype and np.array_equal(f.float().cpu().numpy(), want["feats"]) and np.array_equal(p_.cpu().numpy(), want["pos"])
        made = MaskDesc.make("1d", N, S, want["n_ids"])
        assert torch.equal(desc.desc.cpu(), made.desc) and desc.L == made.L and torch.equal(desc.host_desc(), made.desc) and desc.packable()
        assert cls_tok.tolist() == [[101]] * 7 and sep_tok.tolist() == [[102]] * 7
    out = ops.pair_assemble(bank.txt_ids, bank.txt_len, bank.img_feats, None, torch.tensor(pairs, dtype=torch.int32, device=DEV))
    assert out["pos"] is None and np.array_equal(out["n_ids"].cpu().numpy(), want["n_ids"])
    o = RC.PAIR_VIEW_OFFSET
    unaligned = bank.img_feats.reshape(-1)[o:o + 6 * N * Fd].view(6, N, Fd)       # a bank that is not 16-byte aligned: the narrow copy
    out = ops.pair_assemble(bank.txt_ids, bank.txt_len, unaligned, None, torch.tensor([[5, 0], [0, 1]], dtype=torch.int32, device=DEV))
    assert torch.equal(out["feats"], unaligned[[5, 0]])


# ------------------------------------------------------------------------------------------------ model against the oracle
def _cfg_dict(c):
    return dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)


def _batch(B=4, seed=11):
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, B, N_REG, S_TXT, "1d", seed=seed).items()}
    b["labels"] = torch.tensor([1, 0] * (B // 2))
    return b


def _model(dtype, P):
    m = mv.CXRBertForRetrieval(_cfg_dict(CFG), dtype=dtype, device=DEV)
    m.bert.load_state_dict(P, strict=True)
    m.eval()                                   # dropout off
    return m


def _inputs(b, mask=None):
    return (b["cls_tok"].to(DEV), b["input_txt"].to(DEV), b["attn_mask"].to(DEV) if mask is None else mask, b["segment"].to(DEV),
            (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))


def _reference(P, b):
    """oracle encoder (CPU, f32 autograd) + pooler + ITM head + CrossEntropyLoss -> loss, grads (None where autograd gives none), logits"""
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x, _ = O.encode(Pg, CFG, b["cls_tok"], b["input_txt"], b["attn_mask"], b["segment"], b["img_feats"], b["img_pos"], b["sep_tok"])
    pooled = torch.tanh(F.linear(x[:, 0], Pg["enc.pooler.dense.weight"], Pg["enc.pooler.dense.bias"]))
    logits = F.linear(pooled, Pg["itm.linear.weight"], Pg["itm.linear.bias"])
    loss = torch.nn.CrossEntropyLoss()(logits, b["labels"])
    loss.backward()
    return float(loss.detach()), {k: p.grad for k, p in Pg.items()}, logits.detach()


def _compare_grads(got, ref, rtol):          # as tests/test_classification_gpu.py compares them
    gmax = max(float(g.abs().max()) for g in ref.values())
    floor = (1e-5 if rtol < 1e-3 else 3e-2) * gmax
    for k, r in ref.items():
        g = got[k].float().cpu()
        n = r.double().norm()
        e1 = float((g.double() - r.double()).norm()) / max(float(n), floor * r.numel() ** 0.5)
        assert e1 < rtol, (k, e1, float(n))


@pytest.mark.parametrize("mask", ["dense", "desc"])
@pytest.mark.parametrize("dtype,ltol,rtol", [(torch.float32, 1e-4, 2e-4), (torch.bfloat16, 1e-2, 3e-2)])
def test_loss_logits_and_every_gradient_match_the_oracle(mask, dtype, ltol, rtol):
    P = O.make_params(CFG, seed=3)
    b = _batch()
    assert len(set(b["n_ids"].tolist())) > 1                                       # mixed lengths
    m = _model(dtype, P)
    md = None if mask == "dense" else MaskDesc.make("1d", N_REG, S_TXT, b["n_ids"], DEV)
    loss = m(*_inputs(b, md), labels=b["labels"].to(DEV))
    logits = m.bert.engine.S["itm"].clone()
    loss.backward()
    ref_loss, ref_g, ref_logits = _reference(P, b)
    lerr = float((logits.cpu() - ref_logits).abs().max())
    print(f"retrieval {mask} {dtype}: loss {float(loss.detach()):.6f} oracle {ref_loss:.6f}; logits max-abs err {lerr:.2e}")
    assert abs(float(loss.detach()) - ref_loss) < ltol and lerr < ltol
    got = {k: p.grad for k, p in m.bert.named_parameters()}
    # the parameters without a gradient, by name: the MLM head's own (the model never runs it).  Everything else -- the last layer
    # included, whose non-[CLS] rows are not computed -- has one, in the oracle and here
    unreached = sorted(k for k, g in ref_g.items() if g is None or float(g.abs().max()) == 0.0)
    assert unreached == sorted(k for k in ref_g if k.startswith("mlm.")), unreached
    for k in unreached:
        assert float(got[k].abs().max()) == 0.0, k
    _compare_grads(got, {k: g for k, g in ref_g.items() if k not in unreached}, rtol)
    st = m.stats.cpu()
    assert abs(float(st[0]) / 4 - ref_loss) < ltol and float(st[1]) == 4.0
    if float((ref_logits[:, 1] - ref_logits[:, 0]).abs().min()) > 10 * ltol:
        assert float(st[2]) == float((ref_logits.argmax(1) == b["labels"]).sum())
    with torch.no_grad():                      # without labels: what the model returned before
        assert float((m(*_inputs(b, md)).cpu() - ref_logits).abs().max()) < ltol
        assert float((m.score(*_inputs(b, md)).cpu() - torch.softmax(ref_logits, -1)[:, 1]).abs().max()) < ltol


# ------------------------------------------------------------------------------------------------ fit_step / evaluate / checkpoint
def _bank(m, n, seed, separable=False):
    ids, lens, feats, pos = RC.make_banks(n, n, N_REG, S_TXT, CFG.img_hidden, seed=seed, vocab=CFG.vocab_size)
    if separable:                              # item i: its own token everywhere in the text, its own direction in the features
        rng = np.random.default_rng(seed)
        dirs = rng.standard_normal((n, 1, CFG.img_hidden)).astype(np.float32)
        feats = dirs + 0.05 * feats
        for i in range(n):
            ids[i, :lens[i] - 1] = 200 + i
    bank = RetrievalBank(m)
    bank.add_texts(ids, lens).add_images((torch.from_numpy(feats), torch.from_numpy(pos)))
    return bank


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fit_step_equals_the_three_calls_by_hand(dtype):
    """Both runs enqueue the same kernels on the same inputs; what may differ is the order of f32 additions inside kernels that
    accumulate with atomics (relative 1e-6 of a sum's terms, terms below 1e-3 here).  Adam's first updates are lr g / (|g| + eps), whose
    slope in g is at most lr / eps = lr 1e6: a perturbation of 1e-9 moves a parameter by at most 1e-3 lr."""
    P = O.make_params(CFG, seed=3)
    lr, key = 1e-3, 0x5EED
    idx = torch.tensor([0, 5, 9, 15], dtype=torch.int32)
    ms, losses = [], []
    for fused in (True, False):
        m = _model(dtype, P)
        eng = m.bert.engine
        bank = _bank(m, 16, seed=4)
        ls = []
        for step in (1, 2):
            if fused:
                ls.append(float(m.fit_step(bank, idx, lr, step, key=key)))
            else:
                pairs, labels = ops.pair_negatives(idx.to(DEV), 16, key=key, step=step)
                m.zero_grad()
                loss = m(*bank.assemble(pairs), labels=labels)
                loss.backward()
                eng.check_overflow()
                eng.adamw_step(step, lr=lr, use_scaler=True)
                ls.append(float(loss.detach()))
        ms.append(eng.flat_p.clone())
        losses.append(ls)
    print(f"fit_step {dtype}: losses {losses}; max |dp| {float((ms[0] - ms[1]).abs().max()):.3e}")
    assert max(abs(a - b) for a, b in zip(*losses)) <= 1e-5 * max(losses[0])
    assert float((ms[0] - ms[1]).abs().max()) <= 1e-3 * lr


def test_fit_step_learns_16_separable_items():
    torch.manual_seed(0)
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    m.train()
    bank = _bank(m, 16, seed=8, separable=True)
    idx = torch.arange(16, dtype=torch.int32)
    m.reset_stats()
    losses = torch.stack([m.fit_step(bank, idx, 2e-4, step, key=3) for step in range(1, 21)]).cpu().tolist()       # one read-back
    st = m.stats.cpu()
    print(f"fit_step: loss {losses[0]:.4f} -> {losses[-1]:.4f}; running accuracy {float(st[2] / st[1]):.3f}")
    assert float(st[1]) == 20 * 32 and abs(float(st[0]) / float(st[1]) - sum(losses) / 20) < 1e-4
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5 and losses[-1] < losses[0]
    assert bool(torch.isfinite(m.bert.engine.flat_p).all())


def test_evaluate_equals_score_on_host_built_pairs_then_the_numpy_metrics():
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    eng = m.bert.engine
    bank = _bank(m, 6, seed=5)
    pairs = [(i, t) for i in range(6) for t in range(6)]                           # image i against the 6 texts: 6 groups of C = 6
    labels = [1 if (t == i or (i == 2 and t == 4)) else 0 for i, t in pairs]
    labels[18:24] = [0] * 6                                                        # group 3: no aligned candidate
    eng.training, eng.keep_acts, eng.drop_counter = True, True, 41
    res = m.evaluate(bank, pairs, labels, group_size=6, batch_size=16)             # batches that straddle groups
    assert (eng.training, eng.keep_acts, eng.drop_counter) == (True, True, 41)
    # the path as it was: every pair built on the host, the image side repeated per pair, into score()
    ids, lens = bank.txt_ids.cpu(), bank.txt_len.cpu()
    im, tx = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    desc = MaskDesc.make("1d", N_REG, S_TXT, lens[tx], DEV)
    R_ = len(pairs)
    want_p = m.score(torch.full((R_, 1), 101, device=DEV), ids[tx].to(DEV), desc, torch.ones(R_, S_TXT + 1, dtype=torch.int64, device=DEV),
                     (bank.img_feats[im.to(DEV)], bank.img_pos[im.to(DEV)]), torch.full((R_, 1), 102, device=DEV)).cpu().numpy()
    p = res["p"].cpu().numpy()
    print(f"evaluate: max |p - score| {float(np.abs(p - want_p).max()):.2e}; hits {res['hits']} mrr {res['mrr_score']:.4f} loss {res['eval_loss']:.4f}")
    assert float(np.abs(p - want_p).max()) < 1e-2
    lab = np.asarray(labels)
    want = RC.metrics(p, lab, 6)                                                   # ranks on the kernel's own p
    assert np.array_equal(res["pos"].cpu().numpy(), RC.positions(p, 6)) and res["rank"].cpu().tolist() == want["rank"].tolist()
    assert res["Aligned_lst"] == want["aligned"] and res["groups"] == 6 and res["groups_without_aligned"] == 1
    for q, k in enumerate(RC.KS):
        assert res["hits"][f"R@{k}"] == want["hits"][q]
        assert abs(res["recall"][f"R@{k}"] - want["recall"][q]) <= 2.0 ** -32 and abs(res["precision"][f"R@{k}"] - want["precision"][q]) <= 1e-15
    assert abs(res["mrr_score"] - want["mrr"]) <= 2.0 ** -32
    lp = np.log(np.where(lab == 1, p, 1 - p).astype(np.float64))
    want_loss = np.mean([-lp[s:e].mean() for s, e in R.group_plan(36, 6, 16)[1]])
    assert abs(res["eval_loss"] - want_loss) < 1e-4


def test_evaluate_reads_back_once(monkeypatch):
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    bank = _bank(m, 6, seed=5)
    pairs = torch.tensor([(i, t) for i in range(6) for t in range(6)], dtype=torch.int32)
    labels = (pairs[:, 0] == pairs[:, 1]).to(torch.int32)
    m.evaluate(bank, pairs, labels, group_size=6, batch_size=12)                   # warm: buffers, streams
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(tuple(self.shape)) if self.is_cuda else None, real(self, *a, **k))[1])
    for name in ("item", "tolist", "__bool__", "__float__", "__int__"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda o, nm: lambda self, *a, **k: (calls.append(nm) if self.is_cuda else None, o(self, *a, **k))[1])(orig, name))
    m.evaluate(bank, pairs, labels, group_size=6, batch_size=12)
    monkeypatch.undo()
    assert len(calls) == 1, calls


def test_checkpoint_round_trip(tmp_path):
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    bank = _bank(m, 4, seed=6)
    m.fit_step(bank, torch.arange(4, dtype=torch.int32), 1e-3, 1, key=1)           # a fine-tuned model
    m.eval()
    m.save_pretrained(str(tmp_path / "ret"))
    sd = torch.load(str(tmp_path / "ret" / "pytorch_model.bin"), map_location="cpu")
    assert all(k.startswith(("enc.", "itm.")) for k in sd) and "itm.linear.weight" in sd and "enc.pooler.dense.weight" in sd
    m2 = mv.CXRBertForRetrieval.from_pretrained(str(tmp_path / "ret"), dtype=torch.bfloat16, device=DEV)
    m2.eval()
    args = bank.assemble([(0, 0), (1, 2), (3, 3)])
    with torch.no_grad():
        a, b = m(*args), m2(*args)
    assert torch.equal(a, b) and not torch.equal(m.bert.engine.p["itm.linear.weight"].cpu(), P["itm.linear.weight"].float())


def test_overflowed_backward_is_redone_with_a_smaller_scale():
    """f16 gradient operands under a loss scale far past f16's range: the backward overflows, redoes itself with S / 16 until everything
    is finite and hands over the gradients of a twin run at the default scale."""
    P = O.make_params(CFG, seed=3)
    b = _batch()
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
        grads.append({k: p.grad.detach().float().cpu() for k, p in m.bert.named_parameters()})
    got, twin = grads
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    for k, g in got.items():                                          # as the oracle test: the MLM head's own tensors get none
        if k.startswith("mlm."):
            assert float(g.abs().max()) == 0.0, k
    _compare_grads(got, {k: g for k, g in twin.items() if not k.startswith("mlm.")}, 3e-2)
