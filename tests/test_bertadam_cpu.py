"""medvill_amd.optim.BertAdam host logic (CPU only): constructor rules and refusals, the schedules against the reference fixture's
get_lr() (tests/golden/bertadam.npz), the tensor / chunk tables the kernels run on, the state dict, and the new C-ABI entries."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import medvill_amd as mv
from medvill_amd import _lib
from medvill_amd import hip_ops as ops
from medvill_amd.optim import BertAdam, build_tables, schedule_factor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, max_position_embeddings=128)
NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


def _groups(model, wd=0.01):
    named = list(model.named_parameters())
    return [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": wd},
            {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]


def test_fixture_is_small_and_complete(golden_dir):
    path = os.path.join(golden_dir, "bertadam.npz")
    assert os.path.getsize(path) < 200 * 1024
    z = np.load(path)
    assert set(z["cases"].tolist()) == {"main", "none_grad", "const_lr", "noclip", "constant", "cosine"}
    assert {2, 64, 65} <= set(z["sizes"].tolist()) and all(int(o) % 64 == 0 for o in z["offsets"])
    assert z["main/p"].shape[0] == 8 and float(z["clip_spread"]) < 2e-6
    # one tensor spans more than one kernel chunk and ends on a 1-3 element tail; its gradient is clipped
    big = int(z["big/sizes"][0])
    assert big > ops.OPTIM_CHUNK and big % 4 != 0 and z["big/p"].shape[0] == 2
    assert all(np.sqrt((g[:big].astype(np.float64) ** 2).sum()) > 1.0 for g in z["big/grads"])
    o, s = int(z["offsets"][3]), int(z["sizes"][3])
    norms = np.sqrt((z["grads"][:, o:o + s].astype(np.float64) ** 2).sum(1))
    o5, s5 = int(z["offsets"][5]), int(z["sizes"][5])
    norms5 = np.sqrt((z["grads"][:, o5:o5 + s5].astype(np.float64) ** 2).sum(1))
    assert norms.min() > 1.0 and norms5.max() < 1.0                    # both clip branches
    o1, s1 = int(z["offsets"][1]), int(z["sizes"][1])
    assert not z["grads"][:, o1:o1 + s1].any()                         # the all-zero gradient: the tensor only decays
    assert not np.array_equal(z["main/p"][1][o1:o1 + s1], z["p0"][o1:o1 + s1])


def test_schedules_match_the_reference_get_lr(golden_dir):
    z = np.load(os.path.join(golden_dir, "bertadam.npz"))
    for case in ("main", "const_lr", "noclip", "constant", "cosine"):
        lr, warmup, t_total = [float(v) for v in z[f"{case}/hyper"][:3]]
        sched = str(z[f"{case}/schedule"])
        for s, want in enumerate(z[f"{case}/lr"]):                     # get_lr() after step s: the step count is s + 1
            got = lr if t_total == -1 else lr * schedule_factor(sched, (s + 1) / t_total, warmup)
            assert got == float(want), (case, s, got, want)
    assert schedule_factor("warmup_linear", 0.0, 0.25) == 0.0          # the first step under warm-up moves nothing
    assert schedule_factor("warmup_linear", 2.0, 0.25) == 0            # past t_total: clamped
    assert schedule_factor("warmup_cosine", 0.5, 0.25) == pytest.approx(0.5)
    assert schedule_factor("warmup_linear", 0.5, -1) == 0.25           # warmup = -1: pure linear decay
    with pytest.raises(ValueError):
        schedule_factor("nope", 0.5, 0.1)
    # the optimizer's get_lr(): [0] before the first step, then one value per updated Parameter
    m = mv.CXRBERT(TINY, None, device="cpu")
    opt = BertAdam(m.parameters(), lr=0.01, warmup=0.25, t_total=8)
    assert opt.get_lr() == [0]
    opt._t = 3
    assert opt.get_lr() == [0.01 * (3 / 8 - 1) / (0.25 - 1)] * len(m._plist)


def test_constructor_validation_and_refusals():
    m = mv.CXRBERT(TINY, None, device="cpu")
    for kw in (dict(lr=-1.0), dict(lr=1e-3, schedule="nope"), dict(lr=1e-3, warmup=1.5), dict(lr=1e-3, b1=1.0), dict(lr=1e-3, b2=-0.1),
               dict(lr=1e-3, e=-1.0), dict(lr=1e-3, t_total=0)):
        with pytest.raises(ValueError):
            BertAdam(m.parameters(), **kw)
    opt = BertAdam(_groups(m), lr=1e-3, warmup=0.1, t_total=100)
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["weight_decay"] == 0.0 and opt.defaults["max_grad_norm"] == 1.0
    assert opt.defaults["e"] == 1e-6 and opt.defaults["weight_decay"] == 0.01 and opt.defaults["schedule"] == "warmup_linear"
    g = _groups(m)
    g[1]["lr"] = 5e-4                                                 # groups may differ in weight_decay only
    with pytest.raises(ValueError, match="weight_decay only"):
        BertAdam(g, lr=1e-3)
    g = _groups(m)
    g[1]["weight_decay"] = 0.02                                       # two different positive values
    with pytest.raises(ValueError, match="positive weight_decay"):
        BertAdam(g, lr=1e-3)
    with pytest.raises(ValueError):                                   # not all of the model
        BertAdam(list(m.parameters())[:-1], lr=1e-3)
    with pytest.raises(ValueError):                                   # a foreign Parameter
        BertAdam(list(m.parameters()) + [nn.Parameter(torch.zeros(3))], lr=1e-3)
    with pytest.raises(ValueError):
        BertAdam([nn.Parameter(torch.zeros(3))], lr=1e-3)
    with pytest.raises(ValueError):
        BertAdam([], lr=1e-3)
    # a scheduler scaling one group's lr only is caught at step()
    opt.param_groups[1]["lr"] = 1e-5
    with pytest.raises(RuntimeError, match="diverged"):
        opt._hyper()
    # AdamW is untouched: it still refuses groups
    with pytest.raises(ValueError):
        mv.optim.AdamW(_groups(m), lr=1e-3)


def test_vqa_head_ownership():
    m = mv.CXRBertForVQA(TINY, device="cpu")
    opt = BertAdam(_groups(m), lr=1e-3)
    assert opt._task is m
    assert BertAdam(m.bert.parameters(), lr=1e-3)._task is None
    with pytest.raises(ValueError, match="ALL of its parameters"):
        BertAdam(list(m.bert.parameters()) + [m.ans_classifier[0].weight], lr=1e-3)
    other = mv.CXRBertForVQA(TINY, device="cpu")
    with pytest.raises(ValueError):
        BertAdam(list(m.bert.parameters()) + list(other.ans_classifier.parameters()), lr=1e-3)


def test_build_tables_layout():
    chunk = ops.OPTIM_CHUNK
    tensors, chunks = build_tables([(0, 2, False, True), (64, chunk, True, True), (64 + chunk, 2 * chunk + 1, True, False)])
    assert tensors.dtype == torch.int64 and chunks.dtype == torch.int32
    assert tensors.tolist() == [[0, 2, 0, 2], [64, chunk, 1, 3], [64 + chunk, 2 * chunk + 1, 2, 1]]
    assert chunks.tolist() == [0, 1, 2, 2, 2]
    for bad in ([(32, 4, False, True)], [(0, 0, False, True)], [(0, 100, False, True), (64, 4, False, True)]):
        with pytest.raises(ValueError):
            build_tables(bad)
    src = open(os.path.join(ROOT, "include", "medvill.h")).read()
    assert int(re.search(r"#define MV_OPTIM_CHUNK (\d+)", src).group(1)) == chunk and chunk % 1024 == 0
    assert [ops.SCHEDULE_IDS[k] for k in ("warmup_linear", "warmup_constant", "warmup_cosine")] == [0, 1, 2]


def test_model_tables_follow_the_reference_named_parameters():
    m = mv.CXRBertForVQA(TINY, device="cpu")
    opt = BertAdam(_groups(m), lr=1e-3)
    eng = m.bert.engine
    ent = opt._entries()
    names = m.bert._param_names
    assert len(ent) == len(names) == len(eng.layout)
    by = dict(zip(names, ent))
    # query, key and value: three tensors (three norms) although adjacent in the buffer
    q, k, v = (by[f"enc.encoder.layer.0.attention.self.{n}.weight"] for n in ("query", "key", "value"))
    assert q[1] == k[1] == v[1] == 64 * 64 and k[0] == q[0] + q[1] and v[0] == k[0] + k[1]
    # the tied decoder matrix is the word embedding, once; the aliases of the state dict add no tensor
    assert sum(1 for n in names if n.endswith("word_embeddings.weight")) == 1 and not any("decoder.weight" in n for n in names)
    assert by["enc.txt_embeddings.word_embeddings.weight"][1] == 300 * 64
    # decay flags are the groups'; tensors the VQA graph does not reach are inactive
    for n, (off, cnt, decay, active) in by.items():
        assert decay == (not any(nd in n for nd in NO_DECAY)), n
        assert active == (not n.startswith(("mlm.", "itm.", "enc.pooler."))), n
        assert off == eng.layout[n][0] and cnt == math.prod(eng.layout[n][1])
    # the tables cover exactly the tensors' elements: alignment gaps belong to no chunk
    tensors, chunks = build_tables(ent)
    covered = torch.zeros(eng.n_flat, dtype=torch.int32)
    for c, t in enumerate(chunks.tolist()):
        off, cnt, first, _ = tensors[t].tolist()
        k_ = c - first
        lo = off + k_ * ops.OPTIM_CHUNK
        covered[lo:min(lo + ops.OPTIM_CHUNK, off + cnt)] += 1
    want = torch.zeros(eng.n_flat, dtype=torch.int32)
    for off, shape in eng.layout.values():
        want[off:off + math.prod(shape)] = 1
    assert torch.equal(covered, want) and int((want == 0).sum()) > 0
    # the classifier's own tables: true row count of the padded second layer, everything active
    hent = opt._head_entries()
    assert [e[1] for e in hent] == [128 * 64, 128, 458 * 128, 458] and all(e[3] for e in hent)
    assert [e[2] for e in hent] == [True, False, True, False]
    # the entries are cached; switching a group's decay on or off afterwards rebuilds them (and the device tables made from them)
    assert opt._entries() is ent
    opt.param_groups[1]["weight_decay"] = 0.01
    ent2 = opt._entries()
    assert ent2 is not ent and all(e[2] for e in ent2) and all(e[2] for e in opt._head_entries())
    opt.param_groups[0]["weight_decay"] = opt.param_groups[1]["weight_decay"] = 0.0
    assert not any(e[2] for e in opt._entries())
    # an encoder passed alone is updated whole
    assert all(e[3] for e in BertAdam(m.bert.parameters(), lr=1e-3)._entries())


def test_step_without_gradients_is_a_no_op_and_state_dict_round_trips():
    m = mv.CXRBERT(TINY, None, device="cpu")
    opt = BertAdam(_groups(m), lr=1e-3, warmup=0.1, t_total=50)
    before = m.engine.flat_p.clone()
    opt.zero_grad()
    assert opt.step() is None and opt._t == 0 and torch.equal(m.engine.flat_p, before)       # like the reference: nothing to do
    m._plist[0].grad = torch.zeros_like(m._plist[0])
    with pytest.raises(RuntimeError, match="some Parameters have a gradient"):
        opt.step()
    m.engine.ensure_opt()
    m.engine.flat_m.fill_(0.5)
    opt._t = 7
    sd = opt.state_dict()
    assert sd["step"] == 7 and set(sd) == {"step", "param_groups", "flat_m", "flat_v"} and sd["param_groups"][0]["warmup"] == 0.1
    m2 = mv.CXRBERT(TINY, None, device="cpu")
    opt2 = BertAdam(_groups(m2), lr=1.0)
    opt2.load_state_dict(sd)
    assert opt2._t == 7 and opt2.param_groups[0]["lr"] == 1e-3 and float(m2.engine.flat_m.min()) == 0.5
    big = mv.CXRBERT(dict(TINY, num_hidden_layers=3), None, device="cpu")
    with pytest.raises(ValueError):
        BertAdam(big.parameters(), lr=1.0).load_state_dict(sd)


def test_kernels_refuse_cpu_tensors():
    t, c = build_tables([(0, 64, True, True)])
    x = torch.zeros(64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tensor_sqnorms(x, t, c, torch.zeros(1), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bertadam_step(x, x, x, x, t, c, torch.zeros(1), lr=1e-3, step=0)


def test_new_abi_entries_are_declared_exported_and_prototyped():
    src = open(os.path.join(ROOT, "include", "medvill.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {m_.group(1): len([a for a in m_.group(2).split(",") if a.strip()])
            for m_ in re.finditer(r"\bint\s+(mv_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ("mv_tensor_sqnorms", "mv_bertadam_step"):
        assert name in decl and name in exported and len(_lib.PROTOTYPES[name]) == decl[name]
    assert _lib.ABI_VERSION == 6 and _lib.load().mv_abi_version() == 6          # additive entry points: the version stays
    from medvill_amd import _build
    assert "mv_optim.hip" in _build.SOURCES
    assert mv.optim.BertAdam is BertAdam


# ------------------------------------------------------------------------------------------------ CXRBertForClassification (host logic)
from medvill_amd.classification import CLF_KEYS, clf_layout, metrics  # noqa: E402


def test_classification_class_is_exported_and_shaped():
    assert mv.CXRBertForClassification is mv.classification.CXRBertForClassification and "CXRBertForClassification" in mv.__all__
    m = mv.CXRBertForClassification(TINY, device="cpu", n_classes=14)
    assert isinstance(m.clf, nn.Linear) and tuple(m.clf.weight.shape) == (14, 64) and tuple(m.clf.bias.shape) == (14,)
    lay, n, Cp = clf_layout(64, 14)
    assert Cp == 16 and m.Ap == 16 and m.head_p.numel() == n
    for name, p in zip(CLF_KEYS, m._hplist):
        assert p.data_ptr() == m.head_p.data_ptr() + lay[name][0] * 4
    pad = m._view(m.head_p, "clf.weight", padded=True)[14:]
    assert tuple(pad.shape) == (2, 64) and float(pad.abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        mv.CXRBertForClassification(TINY, device="cpu", task_type="classification")
    m.set_pos_weight([1.0] * 14)
    assert m.pos_weight.dtype == torch.float32 and m.pos_weight.numel() == 14
    with pytest.raises(ValueError):
        m.set_pos_weight([1.0] * 3)
    # BertAdam: the pooler is reached, the MLM / ITM heads are not; the head's own tables hold the true row count
    opt = BertAdam(_groups(m), lr=1e-3)
    assert opt._task is m
    for n_, e in zip(m.bert._param_names, opt._entries()):
        assert e[3] == (not n_.startswith(("mlm.", "itm."))), n_
    assert [e[1] for e in opt._head_entries()] == [14 * 64, 14] and [e[2] for e in opt._head_entries()] == [True, False]
    assert mv.optim.AdamW(m.parameters(), lr=1e-4)._task is m


def test_classification_checkpoint_layout_and_round_trips(tmp_path):
    m = mv.CXRBertForClassification(TINY, device="cpu", n_classes=5)
    sd = m.state_dict()
    assert {"clf.weight", "clf.bias", "enc.txt_embeddings.word_embeddings.weight", "enc.img_embeddings.img_embeddings.weight",
            "enc.encoder.layer.1.output.dense.weight", "enc.pooler.dense.bias"} <= set(sd)
    assert all(k.startswith(("enc.", "clf.")) for k in sd) and not any(k.startswith(("enc.clf.", "enc.img_encoder.")) for k in sd)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.rand_like(p))
    m.save_pretrained(str(tmp_path / "clf"))
    m2 = mv.CXRBertForClassification.from_pretrained(str(tmp_path / "clf"), device="cpu")
    a, b = m.state_dict(), m2.state_dict()
    assert m2.n_classes == 5 and set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the reference's own dict carries an unused enc.clf.* and the image encoder: ignored
    ref_sd = dict(a)
    ref_sd["enc.clf.weight"], ref_sd["enc.img_encoder.model.0.weight"] = torch.zeros(2, 64), torch.zeros(3)
    r = mv.CXRBertForClassification(TINY, device="cpu", n_classes=5).load_state_dict(ref_sd)
    assert not r.missing_keys and not r.unexpected_keys
    # a pretraining checkpoint: encoder loaded, fresh head (main.py:241-242, strict=False)
    pre = mv.CXRBERT(TINY, None, device="cpu")
    with torch.no_grad():
        for p in pre.parameters():
            p.add_(0.5)
    pre.save_pretrained(str(tmp_path / "pre"))
    m3 = mv.CXRBertForClassification.from_pretrained(str(tmp_path / "pre"), device="cpu", n_classes=5)
    for k, v in pre.state_dict().items():
        if k.startswith("enc."):
            assert torch.equal(m3.bert.state_dict()[k], v), k
    fresh = mv.CXRBertForClassification(TINY, device="cpu", n_classes=5)
    assert all(torch.equal(x, y) for x, y in zip(m3._hplist, fresh._hplist))
    with pytest.raises(ValueError):
        mv.CXRBertForClassification.from_pretrained(a)


def test_classification_training_under_several_ranks_is_refused(monkeypatch):
    import torch.distributed as dist
    m = mv.CXRBertForClassification(TINY, device="cpu", n_classes=14)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    B, N, T = 2, 3, 5
    args = (torch.full((B, 1), 101), torch.ones(B, T, dtype=torch.int64), torch.ones(B, N + T + 2, dtype=torch.int64),
            torch.zeros(B, T, dtype=torch.int64), (torch.zeros(B, N, 2048), torch.zeros(B, N, dtype=torch.int64)), torch.full((B, 1), 102))
    with pytest.raises(RuntimeError, match="data-parallel"):
        m(*args, labels=torch.zeros(B, 14))


def test_metrics_against_brute_force_counting():
    g = torch.Generator().manual_seed(3)
    N, C = 40, 5
    p = (torch.rand(N, C, generator=g) * 10).round() / 10            # one decimal: many ties
    t = (torch.rand(N, C, generator=g) < 0.4).float()
    t[:, 4] = 1.0                                                     # a class with one label value scores 0 (main.py:167-171)
    res = metrics(p, t)

    def brute(s, y):
        pos, neg = s[y > 0.5], s[y <= 0.5]
        if len(pos) == 0 or len(neg) == 0:
            return 0.0
        wins = sum((1.0 if a > b else 0.5 if a == b else 0.0) for a in pos.tolist() for b in neg.tolist())
        return wins / (len(pos) * len(neg))
    for c in range(C):
        assert abs(res["auroc_per_class"][c] - brute(p[:, c], t[:, c])) < 1e-12, c
    assert res["auroc_per_class"][4] == 0.0
    assert abs(res["macro_auroc"] - sum(brute(p[:, c], t[:, c]) for c in range(C)) / C) < 1e-12
    assert abs(res["micro_auroc"] - brute(p.reshape(-1), t.reshape(-1))) < 1e-12
    pred, pos = p > 0.5, t > 0.5
    f1s = []
    for c in range(C):
        tp, fp, fn = int((pred[:, c] & pos[:, c]).sum()), int((pred[:, c] & ~pos[:, c]).sum()), int((~pred[:, c] & pos[:, c]).sum())
        f1s.append(2 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) else 0.0)
    TP, FP, FN = int((pred & pos).sum()), int((pred & ~pos).sum()), int((~pred & pos).sum())
    assert abs(res["macro_f1"] - sum(f1s) / C) < 1e-12 and abs(res["micro_f1"] - 2 * TP / (2 * TP + FP + FN)) < 1e-12
    cnt = torch.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)]).float()
    assert metrics(p, t, counters=cnt)["micro_f1"] == res["micro_f1"]       # from device-style counters


def test_multilabel_entry_is_declared_exported_and_prototyped():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "medvill.h")).read(), flags=re.S)
    m_ = re.search(r"\bint\s+mv_bce_multilabel\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert m_ and len([a for a in m_.group(1).split(",") if a.strip()]) == len(_lib.PROTOTYPES["mv_bce_multilabel"])
    assert any(ln.split()[-1] == "mv_bce_multilabel" for ln in out.splitlines() if ln.split())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bce_multilabel(torch.zeros(2, 16), 14, target=torch.zeros(2, 14), loss=torch.zeros(1))
