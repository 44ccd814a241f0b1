"""Attention output without a GPU: a CPU model refuses (there is no fallback), and the options default to the protocol of today."""
import pytest
import torch

import medvill_amd as mv


def _cpu_model():
    return mv.CXRBERT(dict(vocab_size=200, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                           max_position_embeddings=64, layer_norm_eps=1e-12), None, dtype=torch.float32, device="cpu")


def test_options_default_to_no_attention_output():
    m = _cpu_model()
    assert m.output_attentions is False and m.attention_head_mean is False and m.attention_dtype == torch.float32
    assert m.engine.attn_out is None


def test_cpu_model_refuses():
    m = _cpu_model()
    z = torch.zeros((1, 1), dtype=torch.int64)
    args = (z, z, torch.ones((1, 8), dtype=torch.int64), z, (torch.zeros((1, 2, 2048)), torch.zeros((1, 2), dtype=torch.int64)), z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.attention_maps(*args)
    m.output_attentions = True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.enc(*args)
    with pytest.raises(ValueError):
        m._attention_layers([3])
