"""Report generation on the MI355X: the decode kernels of csrc/mv_decode.hip against torch, and CXRBERT.generate against the oracle's
iterated full forward under the seq2seq mask (oracle/cxrbert_oracle.py)."""
import math

import pytest
import torch

import medvill_amd as mv
from medvill_amd import hip_ops as ops
from medvill_amd._lib import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_NONE
from oracle import cxrbert_oracle as O
from oracle import synth

from tests.test_generate_cpu import reference_beam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16_TOL = 1e-2
MASK, EOS, CLS, SEP = 103, 102, 101, 102


# ------------------------------------------------------------------------------------------------ kernels
def _attn_ref(q, kc, vc, slots, slot_row, nk, A, dh):
    R = q.shape[0]
    out = torch.zeros((R, A * dh), dtype=torch.float32, device=q.device)
    for r in range(R):
        s = slots[slot_row[r] if slot_row is not None else r, :nk[r]].long()
        k = kc[s].float().view(-1, A, dh)
        v = vc[s].float().view(-1, A, dh)
        qq = q[r].float().view(A, dh)
        p = torch.softmax(torch.einsum("ad,jad->aj", qq, k) / math.sqrt(dh), dim=-1)
        out[r] = torch.einsum("aj,jad->ad", p, v).reshape(-1)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R,A,nsplit", [(2, 1, 1), (2, 12, 0), (24, 2, 3), (64, 12, 1), (64, 12, 0)])
def test_attn_decode_matches_gather_softmax(dtype, R, A, nsplit):
    g = torch.Generator(device="cpu").manual_seed(R * 31 + A)
    dh = 64
    H = A * dh
    S = 1500
    prefix = 181                                   # shared by the rows of a "sample" (rows in pairs of beams)
    kv = torch.randn((S, 2 * H), generator=g).to(DEV, dtype)
    q = torch.randn((R, 3 * H), generator=g).to(DEV, dtype)
    rows = (R + 1) // 2
    cols = 1100
    slots = torch.randint(prefix * 2, S, (rows, cols), generator=g, dtype=torch.int32)
    slots[:, :prefix] = (torch.arange(rows) // 2 % 2).unsqueeze(1).to(torch.int32) * prefix + torch.arange(prefix, dtype=torch.int32)
    slot_row = (torch.arange(R, dtype=torch.int32) // 2)
    nk = torch.randint(1, cols + 1, (R,), generator=g, dtype=torch.int32)
    nk[0] = 1
    nk[-1] = cols if R > 1 else nk[-1]                          # 1,100: not a multiple of 64, above 1,024
    slots, slot_row, nk = slots.to(DEV), slot_row.to(DEV), nk.to(DEV)
    ctx = torch.empty((R, H), dtype=dtype, device=DEV)
    ws = torch.empty(32 * R * A * (dh + 2), dtype=torch.float32, device=DEV)
    ops.attn_decode(q, kv, kv[:, H:], slots, nk, ctx, R=R, A=A, dh=dh, max_nk=int(nk.max()), ldq=3 * H, ldkv=2 * H, slot_row=slot_row,
                    nsplit=nsplit, ws=ws)
    ref = _attn_ref(q[:, :H], kv[:, :H], kv[:, H:], slots, slot_row.cpu(), nk.cpu(), A, dh)
    tol = 2e-5 if dtype == torch.float32 else (2e-2 if dtype == torch.bfloat16 else 3e-3)
    assert float((ctx.float() - ref).abs().max()) < tol


def test_attn_decode_many_row_heads_split_on_and_off_agree():
    """B*A = 768 row-head pairs (64 rows x 12 heads), forced splits against one pass."""
    g = torch.Generator(device="cpu").manual_seed(3)
    R, A, dh = 64, 12, 64
    H = A * dh
    kv = torch.randn((4000, 2 * H), generator=g).to(DEV, torch.float16)
    q = torch.randn((R, H), generator=g).to(DEV, torch.float16)
    slots = torch.randint(0, 4000, (R, 500), generator=g, dtype=torch.int32).to(DEV)
    nk = torch.randint(300, 501, (R,), generator=g, dtype=torch.int32).to(DEV)
    ws = torch.empty(8 * R * A * (dh + 2), dtype=torch.float32, device=DEV)
    a = torch.empty((R, H), dtype=torch.float16, device=DEV)
    b = torch.empty_like(a)
    ops.attn_decode(q, kv, kv[:, H:], slots, nk, a, R=R, A=A, dh=dh, max_nk=500, ldkv=2 * H, nsplit=1)
    ops.attn_decode(q, kv, kv[:, H:], slots, nk, b, R=R, A=A, dh=dh, max_nk=500, ldkv=2 * H, nsplit=8, ws=ws)
    assert float((a.float() - b.float()).abs().max()) < 3e-3


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N,K", [(768, 768), (2304, 768), (3072, 768), (768, 3072), (30522, 768)])
def test_gemm_rows_matches_matmul(dtype, N, K):
    g = torch.Generator(device="cpu").manual_seed(N + K)
    W = (torch.randn((N, K), generator=g) * 0.05).to(DEV, dtype)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    for i, M in enumerate((1, 2, 7, 16, 64, 128, 256)):
        x = torch.randn((M, K), generator=g).to(DEV, dtype)
        res = torch.randn((M, N), generator=g).to(DEV, dtype)
        prod = x.float() @ W.float().t()
        for epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES):
            if epi == EPI_NONE:
                ref = prod
            elif epi == EPI_BIAS:
                ref = prod + bias
            elif epi == EPI_BIAS_GELU:
                ref = torch.nn.functional.gelu(prod + bias)
            else:
                ref = prod + bias + res.float()
            out_dt = torch.float32 if (epi == EPI_BIAS_RES or (i + epi) % 2) else dtype
            c = torch.empty((M, N), dtype=out_dt, device=DEV)
            ops.gemm_rows(x, W, c, M=M, N=N, K=K, bias=None if epi == EPI_NONE else bias, epi=epi, r=res if epi == EPI_BIAS_RES else None)
            tol = 2e-3 * math.sqrt(K / 768) + (0 if out_dt == torch.float32 else 4e-2)
            err = float((c.float() - ref).abs().max())
            assert err < tol, (M, N, K, epi, out_dt, err)


def test_gemm_rows_k3072_wide():
    g = torch.Generator(device="cpu").manual_seed(9)
    N, K = 30522, 3072
    W = (torch.randn((N, K), generator=g) * 0.03).to(DEV, torch.float16)
    for M in (1, 7, 256):
        x = torch.randn((M, K), generator=g).to(DEV, torch.float16)
        c = torch.empty((M, N), dtype=torch.float32, device=DEV)
        ops.gemm_rows(x, W, c, M=M, N=N, K=K)
        assert float((c - x.float() @ W.float().t()).abs().max()) < 5e-3


def test_logprob_topk_matches_log_softmax_topk():
    g = torch.Generator(device="cpu").manual_seed(4)
    R, V, Vp = 37, 30522, 30528
    x = (torch.randn((R, Vp), generator=g) * 3).to(DEV)
    x[3, 100] = x[3, 200] = x[3, 50] = 40.0            # a three-way tie: lower index first
    x[4, EOS] = 50.0                                    # the best column, penalised below
    for k in (1, 4, 16):
        vals, idx = ops.logprob_topk(x, k, R=R, V=V, ld=Vp)
        lp = torch.log_softmax(x[:, :V].double(), dim=-1)
        rv, ri = torch.topk(lp, k)
        keep = [r for r in range(R) if r != 3]           # (torch's order inside a tie is unspecified)
        assert torch.equal(idx[keep].cpu(), ri[keep].cpu())
        assert float((vals.double() - rv).abs().max()) < 1e-4
        if k >= 3:
            assert idx[3, :3].tolist() == [50, 100, 200]
        assert int(idx[4, 0]) == EOS
        vals, idx = ops.logprob_topk(x, k, R=R, V=V, ld=Vp, eos_penalty_id=EOS)
        lp2 = lp.clone()
        lp2[:, EOS] = -10000.0
        rv, ri = torch.topk(lp2, k)
        assert int(idx[4, 0]) != EOS and int(idx[4, 0]) == int(ri[4, 0])
        assert float((vals.double() - rv).abs().max()) < 1e-4
    vals, idx = ops.logprob_topk(torch.full((2, 40), -1.0, device=DEV), 4, eos_penalty_id=3)
    assert idx.tolist() == [[0, 1, 2, 4]] * 2


# ------------------------------------------------------------------------------------------------ model
def _cd(cfg):
    return dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                intermediate_size=cfg.intermediate, max_position_embeddings=cfg.max_pos)


def _setup(name, B, N, seed=5, dtype=torch.float32):
    cfg = O.CONFIGS[name]
    P = O.make_params(cfg, seed=seed)
    b = synth.make_batch(cfg, B, N, 8, "s2s", seed=seed)
    feats, pos = torch.from_numpy(b["img_feats"]), torch.from_numpy(b["img_pos"])
    model = mv.CXRBERT(_cd(cfg), None, dtype=dtype, device=DEV)
    model.load_state_dict(P)
    model.eval()
    cls = torch.full((B, 1), CLS, dtype=torch.int64)
    sep = torch.full((B, 1), SEP, dtype=torch.int64)
    return cfg, P, model, cls, sep, feats, pos


def _s2s(B, n2, T):
    L = n2 + T
    m = torch.zeros((B, L, L), dtype=torch.int64)
    m[:, :, :n2] = 1
    m[:, n2:, n2:] = torch.tril(torch.ones((T, T), dtype=torch.int64))
    return m


def _oracle_step_logits(P, cfg, cls, sep, feats, pos, prev):
    """MLM logits at text row t = len(prev) of forward([prev..., MASK, pad]) under s2s."""
    B = feats.shape[0]
    n2 = feats.shape[1] + 2
    t = prev.shape[1]
    txt = torch.cat([prev, torch.full((B, 1), MASK, dtype=torch.int64), torch.zeros((B, 1), dtype=torch.int64)], 1)
    seg = torch.ones_like(txt)
    mlm, _ = O.forward(P, cfg, cls, txt, _s2s(B, n2, t + 2), seg, feats, pos, sep)
    return mlm[:, n2 + t]


def test_forced_step_logits_match_oracle_c1_f32_and_16bit():
    B, N, T = 3, 10, 7
    cfg, P, m32, cls, sep, feats, pos = _setup("c1", B, N)
    forced = torch.randint(1000, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(1))
    ref = torch.stack([_oracle_step_logits(P, cfg, cls, sep, feats, pos, forced[:, :t]) for t in range(T)], 1)
    _, lp, logits = m32.generate(cls, (feats, pos), sep, forced_ids=forced)
    assert logits.shape == (B, T, cfg.vocab_size)
    assert float((logits.cpu() - ref).abs().max()) < 1e-3
    assert float((lp.cpu() - torch.log_softmax(ref, -1).gather(2, forced.unsqueeze(2)).squeeze(2)).abs().max()) < 1e-3
    m16 = mv.CXRBERT(_cd(cfg), None, dtype=torch.bfloat16, device=DEV)
    m16.load_state_dict(P)
    m16.eval()
    _, _, l16 = m16.generate(cls, (feats, pos), sep, forced_ids=forced)
    assert float((l16.cpu() - ref).abs().max()) < BF16_TOL


def test_forced_step_logits_match_engine_full_forward_base_16bit():
    B, N, T = 2, 180, 6
    cfg, P, m, cls, sep, feats, pos = _setup("base", B, N, dtype=torch.bfloat16)
    forced = torch.randint(1000, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(2))
    _, _, logits = m.generate(cls, (feats, pos), sep, forced_ids=forced)
    n2 = N + 2
    txt = torch.cat([forced, torch.zeros((B, 1), dtype=torch.int64)], 1)       # full forward: row t sees forced[:t] and itself
    # MASK at row t: run the full s2s forward once per step with forced[:t] + MASK (later positions invisible)
    for t in range(T):
        tt = txt.clone()
        tt[:, t] = MASK
        with torch.no_grad():
            mlm, _ = m(cls, tt, _s2s(B, n2, T + 1), torch.ones_like(tt), (feats, pos), sep)
        err = float((logits[:, t].float() - mlm[:, n2 + t].float()).abs().max())
        assert err < BF16_TOL, (t, err)


def _oracle_greedy(P, cfg, cls, sep, feats, pos, steps):
    B = feats.shape[0]
    prev = torch.zeros((B, 0), dtype=torch.int64)
    margins = []
    for _ in range(steps):
        lg = _oracle_step_logits(P, cfg, cls, sep, feats, pos, prev)
        top2 = torch.topk(lg, 2, dim=-1).values
        margins.append(top2[:, 0] - top2[:, 1])
        prev = torch.cat([prev, lg.argmax(-1, keepdim=True)], 1)
    return prev, torch.stack(margins, 1)


def test_greedy_token_exact_f32_and_16bit_up_to_small_margins():
    B, N, steps = 3, 10, 8
    cfg, P, m32, cls, sep, feats, pos = _setup("c1", B, N)
    ref, margins = _oracle_greedy(P, cfg, cls, sep, feats, pos, steps)
    ids, lp = m32.generate(cls, (feats, pos), sep, max_len=steps)
    assert not bool((ref == EOS).any())                   # random weights: no EOS, every column compares
    assert torch.equal(ids.cpu(), ref)
    m16 = mv.CXRBERT(_cd(cfg), None, dtype=torch.bfloat16, device=DEV)
    m16.load_state_dict(P)
    m16.eval()
    ids16, _ = m16.generate(cls, (feats, pos), sep, max_len=steps)
    for b in range(B):
        for t in range(steps):
            if float(margins[b, t]) < 2 * BF16_TOL:
                break
            assert int(ids16[b, t]) == int(ref[b, t]), (b, t)
    # beam_size = 1 is greedy
    ids1, _ = m32.generate(cls, (feats, pos), sep, max_len=steps, beam_size=1)
    assert torch.equal(ids1, ids)


def test_beam_k4_matches_transcription_on_oracle_logprobs():
    B, N, K, steps = 2, 8, 4, 6
    cfg, P, m, cls, sep, feats, pos = _setup("c1", B, N)
    ids, scores, tr = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=K, return_traces=True)
    # drive the transcription with the oracle: each step's log-probs of every beam's history
    seqs = torch.zeros((B * K, 0), dtype=torch.int64)
    tables = []
    featsK, posK = feats.repeat_interleave(K, 0), pos.repeat_interleave(K, 0)
    clsK, sepK = cls.repeat_interleave(K, 0), sep.repeat_interleave(K, 0)
    for t in range(steps):
        lg = _oracle_step_logits(P, cfg, clsK, sepK, featsK, posK, seqs)
        tables.append(torch.log_softmax(lg, -1))
        _, _, (sc, wids, ptrs) = reference_beam(tables, B, K, EOS, 0, 0.0, steps)
        w, p = torch.tensor(wids[-1]), torch.tensor(ptrs[-1])
        par = (torch.arange(B).unsqueeze(1) * K + p).reshape(-1)
        seqs = torch.cat([seqs[par], w.reshape(-1, 1)], 1)
    ref_ids, ref_best, (sc, wids, ptrs) = reference_beam(tables, B, K, EOS, 0, 0.0, steps)
    assert torch.equal(ids.cpu(), ref_ids)
    assert torch.equal(tr["wids"][:, :steps].cpu().permute(1, 0, 2), torch.tensor(wids))
    assert torch.equal(tr["ptrs"][:, :steps].cpu().permute(1, 0, 2), torch.tensor(ptrs))
    assert float((scores.cpu() - ref_best.float()).abs().max()) < 1e-3


def test_batch_equals_each_sample_alone_and_training_after_generate():
    B, N, steps = 3, 10, 6
    cfg, P, m, cls, sep, feats, pos = _setup("c1", B, N)
    ids, _ = m.generate(cls, (feats, pos), sep, max_len=steps)
    idsk, _ = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=3)
    for b in range(B):
        one, _ = m.generate(cls[b:b + 1], (feats[b:b + 1], pos[b:b + 1]), sep[b:b + 1], max_len=steps)
        assert torch.equal(one[0], ids[b])
        onek, _ = m.generate(cls[b:b + 1], (feats[b:b + 1], pos[b:b + 1]), sep[b:b + 1], max_len=steps, beam_size=3)
        assert torch.equal(onek[0], idsk[b])
    # a training step after generate() gives the loss it gives without it
    batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(cfg, 4, 16, 45, "mixed", seed=5).items()}
    stats = []
    for gen_first in (False, True):
        torch.manual_seed(0)
        mm = mv.CXRBERT(_cd(cfg), None, dtype=torch.bfloat16, device=DEV)
        mm.load_state_dict(P)
        mm.train()
        if gen_first:
            mm.generate(cls, (feats, pos), sep, max_len=4, beam_size=2)
            assert mm.training
        stats.append(mv.TrainStep(mm, lr=1e-5)(dict(batch), train=True).cpu())
    s0, s1 = stats
    assert torch.equal(s0[[1, 2, 4, 5]], s1[[1, 2, 4, 5]])                       # counts, correct predictions
    # the nll sums are fp32 atomicAdd()s of n terms whose order changes from run to run: two runs of the same step may differ by up to n
    # roundings of the sum, n * eps * |sum| (2 ulps of the MLM mean, 1.9e-6, were seen; the mean's own ulp is 9.5e-7)
    eps = torch.finfo(torch.float32).eps
    for i, n in ((0, 1), (3, 4)):
        assert abs(float(s0[i]) - float(s1[i])) <= float(s0[n]) * eps * abs(float(s0[i])), (i, float(s0[i]), float(s1[i]))


def test_more_than_256_rows_per_step():
    """B*K = 136 beams feed 272 rows per step: more than one mv_gemm_rows call per product; batch of 34 x beam 4 equals its halves."""
    B, N, K, steps = 34, 6, 4, 3
    cfg, P, m, cls, sep, feats, pos = _setup("c1", B, N, dtype=torch.bfloat16)
    ids, sc = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=K)
    for h in (slice(0, 17), slice(17, 34)):
        ih, sh = m.generate(cls[h], (feats[h], pos[h]), sep[h], max_len=steps, beam_size=K)
        assert torch.equal(ih, ids[h])
        assert float((sh - sc[h]).abs().max()) < 1e-4
