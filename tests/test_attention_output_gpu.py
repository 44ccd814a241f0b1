"""Attention output of the encoder (model.output_attentions / CXRBERT.attention_maps) on the GPU: a 2-layer model with two heads of
width 64, L = 40 and L = 130 (one and three 64-key tiles, both ragged), the f32 engine (VALU kernel) and the 16-bit engine (MFMA
kernel).  The wiring is checked without a free tolerance: each returned layer against the fp64 softmax restated from the engine's own
stored qkv and the mask, within the per-element bound of tests/attn_probs_cases.py.  The oracle comparison states measured tolerances
(see ORACLE_TOL)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import medvill_amd as mv                                   # noqa: E402
from medvill_amd import hip_ops as ops                     # noqa: E402
from medvill_amd.data import MaskDesc                      # noqa: E402
from oracle import cxrbert_oracle as O                      # noqa: E402
from oracle import synth                                    # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as C                                      # noqa: E402
import attn_probs_cases as P                                # noqa: E402

DEV = "cuda"
CFG = O.OracleConfig(vocab_size=1000, hidden=128, layers=2, heads=2, intermediate=512, max_pos=512)
SHAPES = {40: (8, 29), 130: (16, 111)}                      # L -> (N image regions, S text positions): L = N + S + 3
FAMILIES = ("full", "s2s", "bar", "noncross", "1d")
# max |P - oracle's softmax| over both layers, all five families and both lengths, measured on an MI355X: 5.96e-8 on the f32 engine
# (the oracle is f32 torch on the CPU: one ulp of a probability near 1), 1.26e-5 on the 16-bit engine (f16 forward operands: the
# projections the scores are computed from are f16).  Asserted at twice the measurement rounded up to one digit; the margin absorbs
# another machine's summation order.
ORACLE_TOL = {torch.float32: 2e-7, torch.bfloat16: 3e-5}


def _model(dtype, seed=7):
    torch.manual_seed(1234)                                 # the engine's dropout stream is keyed by torch's seed at construction
    m = mv.CXRBERT(dict(vocab_size=CFG.vocab_size, hidden_size=CFG.hidden, num_hidden_layers=CFG.layers, num_attention_heads=CFG.heads,
                        intermediate_size=CFG.intermediate, max_position_embeddings=CFG.max_pos, layer_norm_eps=CFG.ln_eps),
                   None, dtype=dtype, device=DEV)
    m.load_state_dict(O.make_params(CFG, seed=seed), strict=True)
    m.eval()
    return m


def _batch(L, family, B=2, seed=11):
    N, S = SHAPES[L]
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(CFG, B, N, S, family, seed=seed).items()}
    return b, N, S


def _args(b, mask=None):
    return (b["cls_tok"].to(DEV), b["input_txt"].to(DEV), (b["attn_mask"] if mask is None else mask).to(DEV), b["segment"].to(DEV),
            (b["img_feats"].to(DEV), b["img_pos"].to(DEV)), b["sep_tok"].to(DEV))


def _dense(b):
    m = b["attn_mask"].bool()
    return (m if m.dim() == 3 else m[:, None, :].expand(-1, m.shape[-1], -1)).contiguous()


def _stored_qkv(eng, l, B, L):
    """the layer's fused projection as the attention kernels read it (forward encoding)"""
    H = eng.cfg.hidden
    return eng._ws[f"qkv{l}"][:B * L * 3 * H].view(B, L, 3 * H)


def _enc_name(eng):
    return {torch.float32: C.F32, torch.bfloat16: C.BF16, torch.float16: C.F16}[eng.fadt]


def _pcfg(eng, B, L, p, out, hm):
    return dict(B=B, L=L, A=eng.cfg.heads, dh=eng.cfg.hidden // eng.cfg.heads, p=p, planes=16, out=out, hm=int(hm), enc=_enc_name(eng), path="model")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L", [40, 130])
@pytest.mark.parametrize("family", FAMILIES + ("desc",))
def test_returned_layers_equal_the_softmax_of_the_stored_projections(dtype, L, family):
    """wiring: layers, heads, mask and statistics are the layer's own.  `desc`: the seq2seq family as MaskDesc descriptors."""
    model = _model(dtype)
    eng = model.engine
    b, N, S = _batch(L, "s2s" if family == "desc" else family)
    mask = MaskDesc.make("s2s", N, S, b["n_ids"], device=DEV) if family == "desc" else None
    model.output_attentions = True
    hidden, pooled, attn = model.enc(*_args(b, mask))        # grad mode on: the per-layer projections are kept
    assert isinstance(attn, tuple) and len(attn) == CFG.layers and eng.attn_out is None
    B, A = 2, CFG.heads
    dense = _dense(b).to(DEV)
    for l, probs in enumerate(attn):
        assert probs.shape == (B, A, L, L) and probs.dtype == torch.float32 and not probs.requires_grad
        cfg = _pcfg(eng, B, L, 0.0, C.F32, False)
        R = P.reference(cfg, _stored_qkv(eng, l, B, L).double(), dense, None)
        ratio = P.grade(cfg, probs, R)
        print(f"wiring {dtype} L{L} {family} layer {l}: error / bound {ratio:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_against_the_oracles_softmax(dtype):
    model = _model(dtype)
    Pm = O.make_params(CFG, seed=7)
    worst = 0.0
    for L in (40, 130):
        for family in FAMILIES:
            b, N, S = _batch(L, family)
            got = model.attention_maps(*_args(b))
            seen = []
            real = torch.softmax

            def spy(x, *a, **k):
                y = real(x, *a, **k)
                seen.append(y)
                return y
            torch.softmax = spy
            try:
                with torch.no_grad():
                    O.encode(Pm, CFG, b["cls_tok"], b["input_txt"], b["attn_mask"], b["segment"], b["img_feats"], b["img_pos"], b["sep_tok"])
            finally:
                torch.softmax = real
            assert len(seen) == CFG.layers == len(got)
            for l in range(CFG.layers):
                e = float((got[l].cpu().double() - seen[l].double()).abs().max())
                print(f"oracle {dtype} L{L} {family} layer {l}: max |dP| = {e:.3e}")
                worst = max(worst, e)
    print(f"oracle {dtype}: worst max |dP| = {worst:.3e} (tolerance {ORACLE_TOL[dtype]:.1e})")
    assert worst <= ORACLE_TOL[dtype], (dtype, worst)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L", [40, 130])
def test_train_mode_probabilities_reproduce_the_context(dtype, L):
    """p = 0.1: the returned matrix is the one the context was computed from -- probs . v equals the layer's ctx, which it only can
    when the keep-bits are decoded as the forward decodes them"""
    model = _model(dtype)
    eng = model.engine
    model.train()
    b, N, S = _batch(L, "bar")
    model.output_attentions = True
    _, _, attn = model.enc(*_args(b))
    B, A, H = 2, CFG.heads, CFG.hidden
    p = float(eng.cfg.dropout)
    assert p == 0.1 and eng.S["p_drop"] == p
    ik = C.inv_keep(p, 16)
    dense = _dense(b).to(DEV)
    enc = _enc_name(eng)
    for l, probs in enumerate(attn):
        a_ = eng.S["layers"][l]
        keep = ops.attn_keep_mask(a_["dropbits"], B, L, A)
        qkv64 = _stored_qkv(eng, l, B, L).double()
        r = C.ref_forward(qkv64, dense, A, [L] * B, keep, ik)
        vis = dense[:, None].expand_as(probs)
        dropped = float((probs[vis] == 0).double().mean())
        assert 0.05 < dropped < 0.15, dropped                # the keep-bits were applied: a tenth of the visible entries is gone
        ctx_k = eng._ws[f"ctx{l}"][:B * L * H].view(B, L, H).double()
        ctx_p = C._unheads(probs.double() @ r["v"])
        if enc == C.F32:
            bound = C._unheads(C.flat_bound(C._heads(r["ctx"], A), C.F32, C.F32_TOL["ctx"], 0.0, 1e-3 * float(r["ctx"].abs().max())))
        else:
            bound = C.fwd_bounds(r, enc, [L] * B, ik)[0]
        ratio, at = C.worst_ratio(ctx_p, ctx_k, bound)
        print(f"train {dtype} L{L} layer {l}: |probs.v - ctx| / bound {ratio:.3f}, dropped {dropped:.3f}")
        assert ratio <= 1.0, (l, ratio, at)
        cfg = _pcfg(eng, B, L, p, C.F32, False)
        P.grade(cfg, probs, P.reference(cfg, qkv64, dense, keep))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_head_mean_layer_selection_and_the_16_bit_output(dtype):
    model = _model(dtype)
    eng = model.engine
    b, N, S = _batch(130, "s2s")
    A = CFG.heads
    per_head = model.attention_maps(*_args(b))
    mean = model.attention_maps(*_args(b), head_mean=True)
    assert len(per_head) == len(mean) == CFG.layers
    for ph, hm in zip(per_head, mean):
        assert hm.shape == (2, 130, 130) and hm.dtype == torch.float32
        want = ph.double().mean(dim=1)
        assert bool(((hm.double() - want).abs() <= A * 2.0 ** -24 * want + 2.0 ** -149).all())       # A - 1 additions and one division in f32
    one = model.attention_maps(*_args(b), layers=[1])
    assert len(one) == 1 and torch.equal(one[0], per_head[1])
    both = model.attention_maps(*_args(b), layers=(1, 0))
    assert len(both) == 2 and torch.equal(both[0], per_head[0]) and torch.equal(both[1], per_head[1])          # ascending by layer
    with pytest.raises(ValueError):
        model.attention_maps(*_args(b), layers=[2])
    if dtype != torch.float32:                               # the forward encoding as output encoding: the f32 result rounded once
        enc16 = eng.fadt
        lo = model.attention_maps(*_args(b), dtype=enc16)
        for a16, a32 in zip(lo, per_head):
            assert a16.dtype == enc16 and torch.equal(a16, a32.to(enc16))
    with pytest.raises(ValueError):
        model.attention_maps(*_args(b), dtype=torch.float64)
    # the model options: an iterable of layers, the head mean
    model.output_attentions, model.attention_head_mean = [1], True
    with torch.no_grad():
        _, _, attn = model.enc(*_args(b))
    assert len(attn) == 1 and torch.equal(attn[0], mean[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_default_path_returns_none_and_launches_nothing(dtype, monkeypatch):
    model = _model(dtype)
    calls = []
    real = ops.attn_probs
    monkeypatch.setattr(ops, "attn_probs", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    b, N, S = _batch(40, "full")
    with torch.no_grad():
        out = model.enc(*_args(b))
    assert out[2] is None and not calls and model.engine.S["attn_probs"] == [] and model.engine.attn_out is None
    model.attention_maps(*_args(b), layers=[0])
    assert len(calls) == 1                                    # the counter does see a requested layer


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_train_step_after_attention_maps_is_bit_identical(dtype):
    """attention_maps restores the engine's train / keep-activations / dropout-counter / attention-output state: a training step
    (dropout on) draws the masks it would have drawn without the call, so its loss and its final hidden state are bit-identical.
    One sample with one labelled token: the cross-entropy kernels add each row's loss to the sum with a float atomic, so only a
    one-row sum has a bit pattern that does not depend on the order in which the rows arrive (measured with B = 4: the ITM sum of an
    identical step differed in its last bit, 2.6738229 against 2.6738226); the one row's loss still depends on every dropout mask of
    the encoder."""
    b, N, S = _batch(130, "full", B=1)
    lab = b["txt_labels"]
    first = int((lab[0] != -100).nonzero()[0])
    keep_one = torch.full_like(lab, -100)
    keep_one[0, first] = lab[0, first]
    b["txt_labels"] = keep_one
    stats, hidden = [], []
    for with_maps in (False, True):
        model = _model(dtype)
        model.train()
        eng = model.engine
        if with_maps:
            before = (eng.training, eng.keep_acts, eng.drop_counter, eng.attn_out)
            maps = model.attention_maps(*_args(b))
            assert len(maps) == CFG.layers
            assert (eng.training, eng.keep_acts, eng.drop_counter, eng.attn_out) == before
        ts = mv.TrainStep(model, lr=0.0)
        stats.append(ts(dict(b), train=True).clone())
        hidden.append(eng.S["hidden_f"].clone())
        assert eng.attn_out is None and eng.S["attn_probs"] == [] and float(stats[-1][1]) == 1.0 and float(stats[-1][4]) == 1.0
    torch.cuda.synchronize()
    assert torch.equal(stats[0].view(torch.int32), stats[1].view(torch.int32)), (stats[0].tolist(), stats[1].tolist())
    assert torch.equal(hidden[0], hidden[1])
