"""Checkpoint key maps between the pretraining model (models/train_origin.py:254-266, HF `save_pretrained` layout,
keys as in SURVEY.md Appendix C) and the reference's downstream programs, which rename the keys when they recover a
pretrained model:

  * fine-tuning for report generation / VQA (Downstream_task/report_generation_and_vqa/sc/finetune.py:338-339):
        key.replace('enc.', '').replace('mlm.', 'cls.')
  * decoding (Downstream_task/report_generation_and_vqa/sc/generation_decode.py:385-388), applied to an
    already fine-tuned state dict: prefix the encoder parts with `bert.`.

These are pure renames (no arithmetic); they let checkpoints written by this library's `CXRBERT.save_pretrained`
feed those scripts, and the inverse maps let their checkpoints come back.

`from_hf_bert_keys` is the map the reference gets implicitly when it builds its encoder from a PRETRAINED text BERT
(models/cxrbert_origin.py:41-59: `bert = BertModel.from_pretrained(args.bert_model)`, then `self.txt_embeddings = bert.embeddings`,
`self.encoder = bert.encoder`, `self.pooler = bert.pooler`).
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import torch

WEIGHTS_NAME = "pytorch_model.bin"


def hf_config(cfg, architecture, **extra):
    """The config.json of a model of geometry `cfg` (engine.ModelConfig), HF BertConfig names; `extra`: the task's own entries, last."""
    return dict(architectures=[architecture], model_type="bert", vocab_size=cfg.vocab_size, hidden_size=cfg.hidden,
                num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, intermediate_size=cfg.intermediate,
                max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.ln_eps, hidden_act="gelu",
                hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, **extra)


def write_pretrained(directory, config_dict, state_dict):
    """HF layout: config.json + pytorch_model.bin (train_origin.py:254-266)."""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(config_dict, f, indent=2)
    torch.save({k: v.cpu() for k, v in state_dict.items()}, os.path.join(directory, WEIGHTS_NAME))


def read_config(directory):
    with open(os.path.join(directory, "config.json")) as f:
        return json.load(f)


def read_pretrained(path_or_state_dict, config=None):
    """A checkpoint directory (its config.json is read unless `config` is given) or a state dict (then `config` is required)
    -> (config, state dict)."""
    if not isinstance(path_or_state_dict, (str, os.PathLike)):
        if config is None:
            raise ValueError("from_pretrained(state_dict): pass config= as well")
        return config, path_or_state_dict
    if config is None:
        config = read_config(path_or_state_dict)
    return config, torch.load(os.path.join(path_or_state_dict, WEIGHTS_NAME), map_location="cpu")


def to_finetune_keys(state_dict):
    """finetune.py:338-339."""
    return OrderedDict((k.replace("enc.", "").replace("mlm.", "cls."), v) for k, v in state_dict.items())


def from_finetune_keys(state_dict):
    """Inverse of `to_finetune_keys` for the tensors of the pretraining path."""
    out = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith("cls."):
            out["mlm." + k[4:]] = v
        elif k.startswith(("txt_embeddings.", "img_embeddings.", "img_encoder.", "encoder.", "pooler.")):
            out["enc." + k] = v
        else:
            out[k] = v
    return out


def to_decode_keys(state_dict):
    """generation_decode.py:385-388 (on a fine-tune-style state dict)."""
    out = OrderedDict()
    for k, v in state_dict.items():
        k2 = (k.replace("txt_embeddings", "bert.txt_embeddings").replace("img_embeddings", "bert.img_embeddings")
              .replace("img_encoder.model", "bert.img_encoder.model").replace("encoder.layer", "bert.encoder.layer")
              .replace("pooler", "bert.pooler"))
        k2 = k2.replace("bert.img_embeddings.bert.img_embeddings", "bert.img_embeddings.img_embeddings")
        out[k2] = v
    return out


def from_hf_bert_keys(state_dict):
    """A HF `BertModel` / `BertForPreTraining` state dict (`[bert.]embeddings.* / encoder.layer.* / pooler.*`, TF-era `LayerNorm.gamma /
    beta` accepted) -> the CXRBERT keys those modules live under (cxrbert_origin.py:56-57,72-73): `enc.txt_embeddings.*`,
    `enc.encoder.*`, `enc.pooler.*`.  Everything else of such a checkpoint (its `cls.*` pretraining heads, `position_ids`) is dropped:
    the reference keeps nothing of it either -- its MLM / ITM heads and the image projection start from their own initialisers."""
    out = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith("bert."):
            k = k[5:]
        k = k.replace("LayerNorm.gamma", "LayerNorm.weight").replace("LayerNorm.beta", "LayerNorm.bias")
        if "position_ids" in k or "token_type_ids" in k:
            continue
        if k.startswith("embeddings."):
            out["enc.txt_embeddings." + k[len("embeddings."):]] = v
        elif k.startswith("encoder."):
            out["enc.encoder." + k[len("encoder."):]] = v
        elif k.startswith("pooler."):
            out["enc.pooler." + k[len("pooler."):]] = v
    return out
