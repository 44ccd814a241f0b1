"""CXRBertForVQA host logic (CPU only): export, classifier shapes and initialisation, the reference's VQA state-dict layout
(finetune.py:338-339 + ans_classifier.*), checkpoint round trips, the new C-ABI entries, the optimizer's parameter rules and the
single-rank rule."""
import json
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import medvill_amd as mv
from medvill_amd import _lib
from medvill_amd.checkpoint import to_finetune_keys
from medvill_amd.vqa import HEAD_KEYS, head_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, max_position_embeddings=128)


def test_class_is_exported():
    assert mv.CXRBertForVQA is mv.vqa.CXRBertForVQA
    assert "CXRBertForVQA" in mv.__all__


def test_classifier_shapes_and_init():
    m = mv.CXRBertForVQA(TINY, device="cpu")
    c = m.ans_classifier
    assert isinstance(c, nn.Sequential) and isinstance(c[1], nn.ReLU)
    assert tuple(c[0].weight.shape) == (128, 64) and tuple(c[0].bias.shape) == (128,)
    assert tuple(c[2].weight.shape) == (458, 128) and tuple(c[2].bias.shape) == (458,)
    for w in (c[0].weight, c[2].weight):
        assert abs(float(w.std()) - 0.02) < 2e-3 and abs(float(w.mean())) < 2e-3
    assert float(c[0].bias.abs().max()) == 0.0 and float(c[2].bias.abs().max()) == 0.0
    # the Parameters are views of the classifier's flat buffer; the padding rows of the second layer are zero
    lay, n, Ap = head_layout(64, 458)
    assert Ap == 464 and m.head_p.numel() == n
    for name, p in zip(HEAD_KEYS, m._hplist):
        assert p.data_ptr() == m.head_p.data_ptr() + lay[name][0] * 4
    pad = m._view(m.head_p, HEAD_KEYS[2], padded=True)[458:]
    assert tuple(pad.shape) == (6, 128) and float(pad.abs().max()) == 0.0
    # seeded from torch.initial_seed(): two models agree, reset_head(seed) differs
    m2 = mv.CXRBertForVQA(TINY, device="cpu", n_answers=20)
    assert tuple(m2.ans_classifier[2].weight.shape) == (20, 128) and m2.Ap == 32
    assert torch.equal(m.ans_classifier[0].weight, mv.CXRBertForVQA(TINY, device="cpu").ans_classifier[0].weight)


def test_state_dict_keys_are_the_reference_vqa_layout():
    with open(os.path.join(ROOT, "tests", "golden", "state_manifest.json")) as f:
        man = json.load(f)
    c = man["config"]
    m = mv.CXRBertForVQA(dict(c), dtype=torch.float32, device="cpu")
    want = {k for k in to_finetune_keys({k: None for k in man["keys"]}) if not k.startswith(("cls.", "itm."))} | set(HEAD_KEYS)
    sd = m.state_dict()
    assert set(sd) == want
    shapes = {to_finetune_keys({k: None}).popitem()[0]: v[0] for k, v in man["keys"].items()}
    assert all(list(sd[k].shape) == shapes[k] for k in sd if k in shapes)


def test_save_load_round_trip(tmp_path):
    m = mv.CXRBertForVQA(TINY, device="cpu")
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.rand_like(p))
    m.save_pretrained(str(tmp_path / "vqa"))
    m2 = mv.CXRBertForVQA.from_pretrained(str(tmp_path / "vqa"), device="cpu")
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    m3 = mv.CXRBertForVQA(TINY, device="cpu")
    r = m3.load_state_dict(a)
    assert not r.missing_keys and not r.unexpected_keys
    assert all(torch.equal(v, m3.state_dict()[k]) for k, v in a.items())


def test_from_pretrained_cxrbert_checkpoint_and_vqa_dict(tmp_path):
    pre = mv.CXRBERT(TINY, None, device="cpu")
    with torch.no_grad():
        for p in pre.parameters():
            p.add_(0.5)
    pre.save_pretrained(str(tmp_path / "pre"))
    m = mv.CXRBertForVQA.from_pretrained(str(tmp_path / "pre"), device="cpu")
    for k, v in pre.state_dict().items():
        if k.startswith("enc."):
            assert torch.equal(m.bert.state_dict()[k], v), k
    fresh = mv.CXRBertForVQA(TINY, device="cpu")
    for a_, b_ in zip(m._hplist, fresh._hplist):            # classifier: init_bert_weights seeded from torch.initial_seed()
        assert torch.equal(a_, b_)
    # a reference-layout VQA state dict (finetune keys + ans_classifier.*), as finetune.py saves it
    sd = m.state_dict()
    sd["ans_classifier.2.bias"] = torch.arange(458, dtype=torch.float32)
    m2 = mv.CXRBertForVQA.from_pretrained(sd, config=TINY, device="cpu")
    assert torch.equal(m2.ans_classifier[2].bias, sd["ans_classifier.2.bias"])
    assert torch.equal(m2.bert.state_dict()["enc.encoder.layer.1.output.dense.weight"], sd["encoder.layer.1.output.dense.weight"])
    with pytest.raises(ValueError):
        mv.CXRBertForVQA.from_pretrained(sd)


def _header_decls():
    import re
    src = open(os.path.join(ROOT, "include", "medvill.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(mv_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_new_abi_entries_are_declared_exported_and_prototyped():
    decl = _header_decls()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ("mv_bce_fwd_bwd", "mv_rows_mul"):
        assert name in decl and name in exported and len(_lib.PROTOTYPES[name]) == decl[name]
    assert _lib.ABI_VERSION == 6 and _lib.load().mv_abi_version() == 6
    from medvill_amd import _build
    assert "mv_vqa.hip" in _build.SOURCES


def test_fused_adamw_takes_the_vqa_model_and_still_refuses_foreign_parameters():
    m = mv.CXRBertForVQA(TINY, device="cpu")
    opt = mv.optim.AdamW(m.parameters(), lr=1e-4)
    assert opt._task is m and len(opt.param_groups) == 1
    with pytest.raises(ValueError):
        mv.optim.AdamW(list(m.parameters()) + [nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError):                          # part of the classifier only
        mv.optim.AdamW(list(m.bert.parameters()) + [m.ans_classifier[0].weight])
    other = mv.CXRBertForVQA(TINY, device="cpu")
    with pytest.raises(ValueError):                          # somebody else's classifier
        mv.optim.AdamW(list(m.bert.parameters()) + list(other.ans_classifier.parameters()))
    with pytest.raises(ValueError):
        mv.optim.AdamW(list(m.ans_classifier.parameters()))
    plain = mv.optim.AdamW(m.bert.parameters())              # the encoder alone, as before
    assert plain._task is None


def test_training_under_several_ranks_is_refused(monkeypatch):
    import torch.distributed as dist
    m = mv.CXRBertForVQA(TINY, device="cpu")
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    B, N, T = 2, 3, 5
    args = (torch.full((B, 1), 101), torch.ones(B, T, dtype=torch.int64), torch.ones(B, N + T + 2, dtype=torch.int64),
            torch.zeros(B, T, dtype=torch.int64), (torch.zeros(B, N, 2048), torch.zeros(B, N, dtype=torch.int64)), torch.full((B, 1), 102))
    with pytest.raises(RuntimeError, match="data-parallel"):
        m(*args, ans_labels=torch.zeros(B, 458))
