"""Report generation, host side: the beam-search bookkeeping (medvill_amd.beam) against a literal transcription of the reference's
BertForSeq2SeqDecoder.beam_search (model.py:1239-1467), the slot-table update against a gather, and the new ABI symbols.  CPU only."""
import math

import pytest
import torch

import medvill_amd  # noqa: F401
from medvill_amd import _lib
from medvill_amd.beam import BeamSearch, reorder_slot_table

EOS = 102


def reference_beam(tables, B, K, eos_id, min_len, length_penalty, max_len):
    """The reference's loop and final pick, transcribed: tables[t] = log_softmax of step t's logits, [B*K, V] (step 0: row b*K is
    sample b's single beam)."""
    total_scores, beam_masks, step_ids, step_back_ptrs = [], [], [], []
    for t, lt in enumerate(tables):
        log_scores = lt.clone().view(B * K, 1, -1)
        if len(total_scores) == 0:
            log_scores = log_scores.view(B, K, 1, -1)[:, 0]
        if min_len and (t + 1 <= min_len):
            log_scores[:, :, eos_id].fill_(-10000.0)
        kk_scores, kk_ids = torch.topk(log_scores, k=K)
        if len(total_scores) == 0:
            k_ids = torch.reshape(kk_ids, [B, K])
            back_ptrs = torch.zeros(B, K, dtype=torch.long)
            k_scores = torch.reshape(kk_scores, [B, K])
        else:
            last_eos = torch.reshape(beam_masks[-1], [B * K, 1, 1])
            last_seq_scores = torch.reshape(total_scores[-1], [B * K, 1, 1])
            kk_scores += last_eos * (-10000.0) + last_seq_scores
            kk_scores = torch.reshape(kk_scores, [B, K * K])
            k_scores, k_ids = torch.topk(kk_scores, k=K)
            back_ptrs = torch.div(k_ids, K, rounding_mode="floor")
            kk_ids = torch.reshape(kk_ids, [B, K * K])
            k_ids = torch.gather(kk_ids, 1, k_ids)
        step_back_ptrs.append(back_ptrs)
        step_ids.append(k_ids)
        beam_masks.append(torch.eq(k_ids, eos_id).float())
        total_scores.append(k_scores)
    total_scores = [x.tolist() for x in total_scores]
    step_ids = [x.tolist() for x in step_ids]
    step_back_ptrs = [x.tolist() for x in step_back_ptrs]
    pred, best = [], []
    for b in range(B):
        scores = [x[b] for x in total_scores]
        wids_list = [x[b] for x in step_ids]
        ptrs = [x[b] for x in step_back_ptrs]
        last_frame_id = len(scores) - 1
        for i, wids in enumerate(wids_list):
            if all(wid == eos_id for wid in wids):
                last_frame_id = i
                break
        max_score, frame_id, pos_in_frame = -math.inf, -1, -1
        for fid in range(last_frame_id + 1):
            for i, wid in enumerate(wids_list[fid]):
                if wid == eos_id or fid == last_frame_id:
                    s = scores[fid][i] + length_penalty * (fid + 1)
                    if s > max_score:
                        max_score, frame_id, pos_in_frame = s, fid, i
        if frame_id == -1:
            seq = [0]
        else:
            seq = [wids_list[frame_id][pos_in_frame]]
            for fid in range(frame_id, 0, -1):
                pos_in_frame = ptrs[fid][pos_in_frame]
                seq.append(wids_list[fid - 1][pos_in_frame])
            seq.reverse()
        pred.append(seq + [0] * (max_len - len(seq)))
        best.append(max_score)
    return torch.tensor(pred), torch.tensor(best), (total_scores, step_ids, step_back_ptrs)


def run_helper(tables, B, K, eos_id, min_len, length_penalty, max_len):
    bs = BeamSearch(B, K, eos_id, length_penalty)
    for t, lt in enumerate(tables):
        lp = lt.clone()
        if t < min_len:
            lp[:, eos_id] = -10000.0          # what mv_logprob_topk does with eos_penalty_id
        vals, idx = torch.topk(lp, k=K)
        bs.step(vals, idx)
    return bs.finalize(max_len)


def make_tables(B, K, V, steps, seed, eos_boost):
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(steps):
        x = torch.randn((B * K, V), generator=g) * 2.0
        for b, (t0, amount) in enumerate(eos_boost):
            if t >= t0:
                x[b * K:(b + 1) * K, EOS] += amount
        out.append(torch.log_softmax(x, dim=-1))
    return out


@pytest.mark.parametrize("B,K,min_len,lp,boost,seed", [
    (2, 4, 0, 0.0, [(2, 3.0), (5, 4.0)], 1),
    (3, 3, 3, 0.5, [(0, 6.0), (1, 2.5), (9, 0.0)], 2),          # min_len holds EOS back, sample 0 then ends at once
    (1, 5, 0, -0.3, [(3, 8.0)], 3),                               # every beam reaches EOS: an all-EOS frame
    (4, 2, 1, 1.0, [(1, 1.5), (4, 3.5), (6, 9.0), (0, 0.0)], 4),   # samples finishing at different steps, one never
])
def test_beam_helper_matches_reference_transcription(B, K, min_len, lp, boost, seed):
    V, steps = 150, 10
    tables = make_tables(B, K, V, steps, seed, boost)
    ids_r, best_r, (sc_r, wid_r, ptr_r) = reference_beam(tables, B, K, EOS, min_len, lp, steps)
    ids_h, best_h, tr = run_helper(tables, B, K, EOS, min_len, lp, steps)
    assert torch.equal(ids_h, ids_r)
    assert torch.allclose(best_h, best_r.float(), atol=1e-5)
    assert torch.equal(tr["pred_seq"], ids_r)
    assert torch.allclose(tr["scores"].permute(1, 0, 2)[:steps], torch.tensor(sc_r), atol=1e-5)
    assert torch.equal(tr["wids"].permute(1, 0, 2)[:steps], torch.tensor(wid_r))
    assert torch.equal(tr["ptrs"].permute(1, 0, 2)[:steps], torch.tensor(ptr_r))


def test_beam_min_len_and_early_eos_are_exercised():
    """The cases above do reach EOS: an early-EOS beam exists and the min_len steps hold no EOS."""
    tables = make_tables(3, 3, 150, 10, 2, [(0, 6.0), (1, 2.5), (9, 0.0)])
    _, _, tr = run_helper(tables, 3, 3, EOS, 3, 0.5, 10)
    w = tr["wids"]
    assert not bool((w[:, :3] == EOS).any())
    assert bool((w[0, 3:] == EOS).any())


def test_all_done_means_an_all_eos_frame_for_every_sample():
    bs = BeamSearch(2, 2, EOS)
    bs.step(torch.tensor([[-0.1, -0.2], [0, 0], [-0.1, -0.3], [0, 0]]), torch.tensor([[EOS, 5], [0, 0], [EOS, 6], [0, 0]]))
    assert not bool(bs.all_done())
    bs.step(torch.tensor([[-0.1, -0.2]] * 4), torch.tensor([[EOS, 7]] * 4))
    # sample candidates: beams ending in EOS are pushed down by -10000, so the best two extend the non-EOS beam
    assert not bool(bs.all_done())
    bs.ids.append(torch.tensor([[EOS, EOS], [EOS, EOS]]))
    bs.eos_masks.append(torch.ones(2, 2))
    assert bool(bs.all_done())


def test_slot_table_reorder_matches_a_gather():
    g = torch.Generator().manual_seed(0)
    B, K, n2, cols = 3, 4, 5, 12
    tbl = torch.randint(0, 1000, (B * K, cols), generator=g, dtype=torch.int32)
    back = torch.randint(0, K, (B, K), generator=g)
    bs = BeamSearch(B, K, EOS)
    parents = bs.parents(back)
    assert torch.equal(parents, (torch.arange(B).unsqueeze(1) * K + back).reshape(-1))
    for t in (0, 1, 4):
        ref = tbl.clone()
        ref[:, n2:n2 + t] = tbl[parents][:, n2:n2 + t]
        got = reorder_slot_table(tbl.clone(), parents, n2, n2 + t)
        assert torch.equal(got, ref)
        assert torch.equal(got[:, :n2], tbl[:, :n2]) and torch.equal(got[:, n2 + t:], tbl[:, n2 + t:])


def test_new_abi_symbols_are_declared_and_exported():
    import ctypes
    from tests.test_abi import header_functions
    decl = header_functions()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in (("mv_gemm_rows", 17), ("mv_attn_decode", 20), ("mv_logprob_topk", 10), ("mv_embed_rows", 18)):
        assert decl.get(name) == n and len(_lib.PROTOTYPES[name]) == n
        assert hasattr(raw, name)
    assert _lib.load().mv_abi_version() == 6


def test_generate_refuses_ngram_blocking():
    from medvill_amd.generate import generate

    class Fake:
        pass
    with pytest.raises(NotImplementedError):
        generate(Fake(), None, None, None, forbid_duplicate_ngrams=True)


def test_cpu_model_refuses_generation():
    import medvill_amd as mv
    cd = dict(vocab_size=200, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128, max_position_embeddings=64)
    m = mv.CXRBERT(cd, None, dtype=torch.float32, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(torch.full((1, 1), 101), (torch.zeros(1, 2, 2048), torch.zeros(1, 2, dtype=torch.int64)), torch.full((1, 1), 102), max_len=4)
