"""Report fine-tuning from a device-resident bank on the MI355X: CXRBertForReportFinetune.fit_step / eval_step over a data.ReportBank
against the host-list route -- the same model fed the batch and the prediction lists that the numpy restatement of
tests/report_bank_cases.py builds for the same draws.  The tiny configuration and the shapes are those of test_report_finetune_gpu.py,
and so are the tolerances: LTOL on a loss (1e-4 f32, 1e-2 16-bit) and RTOL on a gradient by that file's norm-relative measure (2e-4 f32,
3e-2 16-bit; the step's f32 atomics rule out bitwise equality there).  A forward without dropout issues the same launches on the same
plan in both routes: its loss is compared for equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                     # noqa: E402
from oracle import cxrbert_oracle as O       # noqa: E402
from oracle import synth                     # noqa: E402
import report_bank_cases as C                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = O.CONFIGS["c1"]
N_REG, S_TXT, BATCH, MAX_PRED, N_ITEMS = 16, 45, 4, 4, 6
T_TXT = S_TXT + 1
IDX = [3, 0, 5, 3]                           # a repeated item
LTOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2, torch.float16: 1e-2}
RTOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2, torch.float16: 3e-2}
UNREACHED = ("itm.", "enc.pooler.")
FAMILY_OF = {"s2s": "s2s", "bi": "1d", "bar": "bar"}


def _cfg_dict(c, **over):
    d = dict(vocab_size=c.vocab_size, hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads,
             intermediate_size=c.intermediate, max_position_embeddings=c.max_pos, layer_norm_eps=c.ln_eps)
    d.update(over)
    return d


def _model(dtype, P, ls=0.1, cfg=None, **kw):
    if dtype == torch.bfloat16:
        kw = dict(fwd_operand="bf16", grad_operand="bf16", **kw)
    m = mv.CXRBertForReportFinetune(cfg or _cfg_dict(CFG), dtype=torch.float32 if dtype == torch.float32 else torch.bfloat16, device=DEV,
                                    label_smoothing=ls, **kw)
    if P is not None:
        m.bert.load_state_dict(P, strict=True)
    m.eval()
    return m


_SRC = {}


def _source():
    """The data set: N_ITEMS reports (tokens + [SEP] + [PAD]..., lengths counting the [SEP]) and their region features."""
    if not _SRC:
        b = synth.make_batch(CFG, N_ITEMS, N_REG, S_TXT, "s2s", seed=11)
        _SRC.update(ids=b["input_txt"], lens=b["n_ids"], feats=b["img_feats"], pos=b["img_pos"])
    return _SRC


def _bank(m):
    s = _source()
    bank = mv.data.ReportBank(m, max_pred=MAX_PRED)
    bank.add_reports(torch.from_numpy(s["ids"]), torch.from_numpy(s["lens"]))
    bank.add_images((torch.from_numpy(s["feats"]), torch.from_numpy(s["pos"])))
    return bank


def _host_batch(bank, words, mode, how):
    """What the host-list route feeds the model: the restatement's batch and lists for `words`, the features in the bank's encoding."""
    s = _source()
    np_bank = dict(txt_ids=s["ids"], txt_len=s["lens"].astype(np.int32), img_pos=s["pos"],
                   n_pred=np.array([C.n_pred_of(int(ln), MAX_PRED) for ln in s["lens"]], np.int32),
                   img_feats=bank.img_feats.float().cpu().numpy())
    modes = [mode] * BATCH if isinstance(mode, str) else list(mode)
    r = C.assemble(np_bank, IDX, MAX_PRED, words, family=[mv.data.FAMILY_ID[FAMILY_OF[m_]] for m_ in modes])
    n_ids = torch.from_numpy(s["lens"][IDX])
    if how == "desc":
        mask = mv.data.MaskDesc.make([FAMILY_OF[m_] for m_ in modes], N_REG, S_TXT, n_ids, DEV)
    else:
        assert isinstance(mode, str)
        mask = mv.data.build_mask(FAMILY_OF[mode], N_REG, S_TXT, n_ids, DEV)
    args = (torch.full((BATCH, 1), 101, dtype=torch.int64, device=DEV), torch.from_numpy(r["input_txt"]).to(DEV), mask,
            torch.from_numpy(r["segment"]).to(DEV),
            (torch.from_numpy(r["feats"]).to(DEV, bank.feat_dtype), torch.from_numpy(r["pos"]).to(DEV)),
            torch.full((BATCH, 1), 102, dtype=torch.int64, device=DEV))
    lists = {k: torch.from_numpy(r[k]) for k in ("masked_lm_labels", "masked_pos", "masked_weights")}
    return args, lists


def _compare_grads(got, ref, rtol):
    """test_report_finetune_gpu.py's measure: per tensor, |got - ref| / max(|ref|, floor sqrt(numel)) in the 2-norm."""
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


@pytest.mark.parametrize("mode", ["s2s", "bi", "bar"])
@pytest.mark.parametrize("dtype,how", [(torch.float32, "dense"), (torch.float32, "desc"), (torch.bfloat16, "dense"), (torch.bfloat16, "desc"),
                                       (torch.float16, "dense"), (torch.float16, "desc")])
def test_eval_step_equals_the_host_list_route(dtype, how, mode):
    P = O.make_params(CFG, seed=3)
    m = _model(dtype, P)
    bank = _bank(m)
    words = C.injected_draws(BATCH, T_TXT, 5)
    state = (m.bert.engine.training, m.bert.engine.keep_acts, m.bert.engine.drop_counter)
    got = m.eval_step(bank, IDX, step=1, mode=mode, draws=torch.from_numpy(words.astype(np.int64)))
    assert (m.bert.engine.training, m.bert.engine.keep_acts, m.bert.engine.drop_counter) == state and got.grad_fn is None
    stats = m.lm_stats.cpu()
    args, lists = _host_batch(bank, words, mode, how)
    with torch.no_grad():
        want, _ = m(*args, **lists)
    print(f"{dtype} {how} {mode}: eval_step {float(got):.8f} host lists {float(want):.8f}")
    assert float(got) == float(want)
    assert torch.equal(stats, m.lm_stats.cpu())


def test_eval_step_with_one_mode_per_sample_and_hash_draws():
    P = O.make_params(CFG, seed=3)
    m = _model(torch.float16, P)
    bank = _bank(m)
    modes = ["s2s", "bi", "bar", "s2s"]
    got = m.eval_step(bank, IDX, step=7, key=99, mode=modes)
    args, lists = _host_batch(bank, C.draws(99, 7, BATCH, T_TXT), modes, "desc")
    with torch.no_grad():
        want, _ = m(*args, **lists)
    assert float(got) == float(want)
    other = m.eval_step(bank, IDX, step=8, key=99, mode=modes)                # another step: another draw
    assert float(other) != float(got)
    on_dev = m.eval_step(bank, torch.tensor(IDX, dtype=torch.int32, device=DEV), step=7, key=99, mode=modes)
    assert float(on_dev) == float(got)                                        # idx on the device: clamped by the kernel, same batch


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gradients_after_a_backward_match_the_host_list_route(dtype):
    P = O.make_params(CFG, seed=3)
    words = C.injected_draws(BATCH, T_TXT, 5)
    m = _model(dtype, P)                                                   # eval mode: no dropout, the two backwards see one forward
    bank = _bank(m)
    opt = mv.optim.BertAdam(m.parameters(), lr=0.0, weight_decay=0.0)       # lr 0: the step moves nothing, the gradients stay
    loss = m.fit_step(bank, IDX, opt, step=1, draws=torch.from_numpy(words.astype(np.int64)))
    got = {k: p.grad.detach().clone() for k, p in m.bert.named_parameters() if p.grad is not None}
    args, lists = _host_batch(bank, words, "s2s", "desc")
    opt.zero_grad()
    want_loss, _ = m(*args, **lists)
    want_loss.backward()
    ref = {k: p.grad.detach().float().cpu() for k, p in m.bert.named_parameters()
           if p.grad is not None and not k.startswith(UNREACHED)}
    assert float(loss) == float(want_loss.detach()) and len(ref) > 30
    worst = _compare_grads(got, ref, RTOL[dtype])
    print(f"{dtype}: worst gradient error {worst:.2e}")
    for k in got:
        if k.startswith(UNREACHED):
            assert float(got[k].abs().max()) == 0.0, k


def _fit(m, bank, steps, key, generate_first=False):
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    s = _source()
    out = []
    for i in range(steps):
        if generate_first and i == 1:
            f = torch.from_numpy(s["feats"][IDX]).to(DEV)
            m.generate(torch.full((BATCH, 1), 101, dtype=torch.int64, device=DEV), (f, torch.from_numpy(s["pos"][IDX]).to(DEV)),
                       torch.full((BATCH, 1), 102, dtype=torch.int64, device=DEV), max_len=6)
        loss = m.fit_step(bank, IDX, opt, step=i, key=key)
        out.append((float(loss), dict(m.bert.engine.S["drop_keys"]), m.bert.engine.drop_counter))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_three_fit_steps_follow_the_hand_written_loop(dtype):
    P = O.make_params(CFG, seed=3)
    torch.manual_seed(0)
    m = _model(dtype, P)
    bank = _bank(m)
    got = [l for l, _, _ in _fit(m, bank, 3, key=21)]
    torch.manual_seed(0)
    m2 = _model(dtype, P)
    m2.train()
    opt = mv.optim.BertAdam(m2.parameters(), lr=1e-3, weight_decay=0.01)
    want = []
    for i in range(3):                                                     # finetune.py:443-451 with host lists
        args, lists = _host_batch(bank, C.draws(21, i, BATCH, T_TXT), "s2s", "desc")
        opt.zero_grad()
        loss, _ = m2(*args, **lists, drop_worst_ratio=0.0)
        loss.backward()
        opt.step()
        want.append(float(loss))
    print(f"{dtype}: fit_step {got} loop {want}")
    assert got[0] == want[0]                                               # the first step: the same launches on the same parameters
    for a, b in zip(got, want):
        assert abs(a - b) < LTOL[dtype], (got, want)


def test_three_fit_steps_leave_the_unreached_tensors_alone_and_lower_the_loss():
    P = O.make_params(CFG, seed=3)
    torch.manual_seed(0)
    m = _model(torch.bfloat16, P)
    bank = _bank(m)
    words = torch.from_numpy(C.injected_draws(BATCH, T_TXT, 5).astype(np.int64))
    first = float(m.eval_step(bank, IDX, step=0, draws=words))
    before = {k: p.detach().clone() for k, p in m.bert.named_parameters()}
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    for i in range(3):
        m.fit_step(bank, IDX, opt, step=i, draws=words)
    moved = 0
    for k, p in m.bert.named_parameters():
        if k.startswith(UNREACHED):
            assert torch.equal(p.detach(), before[k]), k
        else:
            moved += int(not torch.equal(p.detach(), before[k]))
    assert moved > 10
    assert m.training                                                      # eval_step runs in eval mode whatever the module's mode
    after = float(m.eval_step(bank, IDX, step=0, draws=words))
    assert after < first, (after, first)


def test_a_fit_step_after_generate_draws_the_same_dropout_masks():
    P = O.make_params(CFG, seed=3)
    runs = []
    for gen in (False, True):
        torch.manual_seed(0)
        m = _model(torch.bfloat16, P)
        runs.append(_fit(m, _bank(m), 2, key=4, generate_first=gen))
    for (l0, k0, c0), (l1, k1, c1) in zip(*runs):
        assert k0 == k1 and c0 == c1
    assert runs[0][0][0] == runs[1][0][0] and abs(runs[0][1][0] - runs[1][1][0]) < 1e-3 * abs(runs[0][1][0])


def test_refusals(monkeypatch):
    P = O.make_params(CFG, seed=3)
    m = _model(torch.bfloat16, P)
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3)
    s = _source()
    bank = mv.data.ReportBank(m, max_pred=MAX_PRED)
    with pytest.raises(ValueError, match="empty"):
        m.fit_step(bank, IDX, opt, step=0)
    bank.add_reports(torch.from_numpy(s["ids"]), torch.from_numpy(s["lens"]))
    with pytest.raises(ValueError, match="empty"):
        m.eval_step(bank, IDX, step=0)
    bank.add_images((torch.from_numpy(s["feats"][:4]), torch.from_numpy(s["pos"][:4])))
    with pytest.raises(ValueError, match="6 reports"):                      # unequal halves
        m.fit_step(bank, IDX, opt, step=0)
    bank.add_images((torch.from_numpy(s["feats"][4:]), torch.from_numpy(s["pos"][4:])))
    with pytest.raises(IndexError):
        m.fit_step(bank, [0, N_ITEMS], opt, step=0)
    with pytest.raises(IndexError):
        m.eval_step(bank, [-1, 2], step=0)
    with pytest.raises(ValueError, match="drop_worst_ratio"):
        m.fit_step(bank, IDX, opt, step=0, drop_worst_ratio=1.5)
    short = _model(torch.bfloat16, None, cfg=_cfg_dict(CFG, max_position_embeddings=N_REG + T_TXT + 1))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        short.eval_step(bank, IDX, step=0)
    # a label outside the vocabulary is a bad entry: counted on the device, refused before the encoder runs
    ids = torch.from_numpy(s["ids"]).clone()
    ids[3, :int(s["lens"][3]) - 1] = CFG.vocab_size + 5
    spoiled = mv.data.ReportBank(m, max_pred=MAX_PRED)
    spoiled.add_reports(ids, torch.from_numpy(s["lens"])).add_images((torch.from_numpy(s["feats"]), torch.from_numpy(s["pos"])))
    words = C.injected_draws(BATCH, T_TXT, 5, "equal")
    with pytest.raises(ValueError, match="refused"):
        m.eval_step(spoiled, IDX, step=0, draws=torch.from_numpy(words.astype(np.int64)))
    # several ranks: a gradient step is refused before anything runs
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="data-parallel"):
        m.fit_step(bank, IDX, opt, step=0)
