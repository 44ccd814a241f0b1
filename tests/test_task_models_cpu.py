"""What the task models share (CPU only): the single-rank rule of every fine-tuning entry point, and the checkpoint files
`save_pretrained` writes -- config.json key by key and in order, pytorch_model.bin by its tensor names."""
import json

import pytest
import torch

import medvill_amd as mv

TINY = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, max_position_embeddings=128)
B, N, T = 2, 3, 5


def _args():
    return (torch.full((B, 1), 101), torch.ones(B, T, dtype=torch.int64), torch.ones(B, N + T + 2, dtype=torch.int64),
            torch.zeros(B, T, dtype=torch.int64), (torch.zeros(B, N, 2048), torch.zeros(B, N, dtype=torch.int64)), torch.full((B, 1), 102))


def _report_lists():
    return dict(masked_lm_labels=torch.ones(B, 2, dtype=torch.int64), masked_pos=torch.full((B, 2), N + 3), masked_weights=torch.ones(B, 2))


TASKS = {
    "vqa": (lambda: mv.CXRBertForVQA(TINY, device="cpu"), lambda: dict(ans_labels=torch.zeros(B, 458))),
    "classification": (lambda: mv.CXRBertForClassification(TINY, device="cpu", n_classes=14), lambda: dict(labels=torch.zeros(B, 14))),
    "report": (lambda: mv.CXRBertForReportFinetune(TINY, device="cpu"), _report_lists),
    "retrieval": (lambda: mv.CXRBertForRetrieval(TINY, device="cpu"), lambda: dict(labels=torch.zeros(B, dtype=torch.int64))),
}


@pytest.mark.parametrize("task", sorted(TASKS))
def test_training_under_several_ranks_is_refused(monkeypatch, task):
    import torch.distributed as dist
    make, labels = TASKS[task]
    m = make()
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    assert torch.is_grad_enabled()
    with pytest.raises(RuntimeError, match="data-parallel"):
        m(*_args(), **labels())
    if task == "retrieval":                    # the fused step bypasses autograd: refused before it looks at the bank
        with pytest.raises(RuntimeError, match="data-parallel"):
            m.fit_step(None, torch.zeros(2, dtype=torch.int32), 1e-3, 1)


# ------------------------------------------------------------------------------------------------ checkpoint files
_BASE = [("model_type", "bert"), ("vocab_size", 300), ("hidden_size", 64), ("num_hidden_layers", 2), ("num_attention_heads", 2),
         ("intermediate_size", 128), ("max_position_embeddings", 128), ("type_vocab_size", 2), ("layer_norm_eps", 1e-12),
         ("hidden_act", "gelu"), ("hidden_dropout_prob", 0.1), ("attention_probs_dropout_prob", 0.1)]


def _config(architecture, *extra):
    return [("architectures", [architecture])] + _BASE + list(extra)


_LAYER = ["attention.output.LayerNorm.bias", "attention.output.LayerNorm.weight", "attention.output.dense.bias",
          "attention.output.dense.weight", "attention.self.key.bias", "attention.self.key.weight", "attention.self.query.bias",
          "attention.self.query.weight", "attention.self.value.bias", "attention.self.value.weight", "intermediate.dense.bias",
          "intermediate.dense.weight", "output.LayerNorm.bias", "output.LayerNorm.weight", "output.dense.bias", "output.dense.weight"]
_ENC = ([f"encoder.layer.{i}.{k}" for i in range(2) for k in _LAYER]
        + ["img_embeddings.LayerNorm.bias", "img_embeddings.LayerNorm.weight", "img_embeddings.img_embeddings.bias",
           "img_embeddings.img_embeddings.weight", "img_embeddings.position_embeddings.weight",
           "img_embeddings.token_type_embeddings.weight", "pooler.dense.bias", "pooler.dense.weight",
           "txt_embeddings.LayerNorm.bias", "txt_embeddings.LayerNorm.weight", "txt_embeddings.position_embeddings.weight",
           "txt_embeddings.token_type_embeddings.weight", "txt_embeddings.word_embeddings.weight"])
_MLM = ["predictions.bias", "predictions.decoder.weight", "predictions.transform.LayerNorm.bias",
        "predictions.transform.LayerNorm.weight", "predictions.transform.dense.bias", "predictions.transform.dense.weight"]
_ITM = ["itm.linear.bias", "itm.linear.weight"]


def _keys(enc="", mlm=None, itm=False, head=()):
    return sorted([enc + k for k in _ENC] + ([mlm + k for k in _MLM] if mlm else []) + (_ITM if itm else []) + list(head))


# recorded literals: the two files are a format that other programs (and earlier checkpoints' readers) depend on
CHECKPOINTS = {
    "CXRBERT": (lambda: mv.CXRBERT(TINY, device="cpu"), _config("CXRBERT"), _keys("enc.", "mlm.", itm=True)),
    "CXRBertForVQA": (lambda: mv.CXRBertForVQA(TINY, device="cpu"), _config("CXRBertForVQA", ("n_answers", 458)),
                      _keys(head=mv.vqa.HEAD_KEYS)),
    "CXRBertForClassification": (lambda: mv.CXRBertForClassification(TINY, device="cpu", n_classes=14),
                                 _config("CXRBertForClassification", ("n_classes", 14)), _keys("enc.", head=mv.classification.CLF_KEYS)),
    "CXRBertForReportFinetune": (lambda: mv.CXRBertForReportFinetune(TINY, device="cpu", label_smoothing=0.1),
                                 _config("CXRBertForReportFinetune", ("label_smoothing", 0.1)), _keys("", "cls.", itm=True)),
    "CXRBertForRetrieval": (lambda: mv.CXRBertForRetrieval(TINY, device="cpu"), _config("CXRBertForRetrieval"), _keys("enc.", itm=True)),
}


@pytest.mark.parametrize("name", sorted(CHECKPOINTS))
def test_save_pretrained_writes_the_recorded_files(tmp_path, name):
    make, config, keys = CHECKPOINTS[name]
    make().save_pretrained(str(tmp_path))
    text = (tmp_path / "config.json").read_text()
    got = json.loads(text)
    assert got == dict(config) and list(got) == [k for k, _ in config]
    assert text == json.dumps(dict(config), indent=2)
    assert sorted(torch.load(str(tmp_path / "pytorch_model.bin"), map_location="cpu")) == keys
