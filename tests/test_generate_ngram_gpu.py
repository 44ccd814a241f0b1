"""CXRBERT.generate with n-gram blocking on the MI355X (no_repeat_ngram_size / no_repeat_ignore_ids) against the
plain-Python rule of tests/ngram_cases.py driven by the CPU oracle's log-probs of every beam's history, as
tests/test_generate_gpu.py::test_beam_k4_matches_transcription_on_oracle_logprobs drives the unblocked transcription.  All on the
c1 model, B <= 3, K <= 4, at most 12 steps."""
import pytest
import torch

import medvill_amd as mv

import ngram_cases as C
from tests.test_generate_gpu import BF16_TOL, CLS, DEV, EOS, SEP, _cd, _oracle_greedy, _oracle_step_logits, _setup  # noqa: F401

pytestmark = pytest.mark.gpu
GREEDY_SEED, GREEDY_N, GREEDY_STEPS = 6, 2, 12       # chosen on the CPU: the oracle's unblocked greedy output repeats a bigram (asserted below)


def oracle_blocked_beam(P, cfg, cls, sep, feats, pos, K, steps, n, ignore=None, min_len=0, length_penalty=0.0):
    """The restated search on the oracle's log-probs: every step's table holds the log-probs of the B*K histories the search has
    reached.  -> (ids, best, traces, smallest margin between a chosen candidate and the next one over all steps)."""
    B = feats.shape[0]
    seqs = torch.zeros((B * K, 0), dtype=torch.int64)
    featsK, posK = feats.repeat_interleave(K, 0), pos.repeat_interleave(K, 0)
    clsK, sepK = cls.repeat_interleave(K, 0), sep.repeat_interleave(K, 0)
    tables, margin = [], float("inf")
    for t in range(steps):
        lg = _oracle_step_logits(P, cfg, clsK, sepK, featsK, posK, seqs)
        tables.append(torch.log_softmax(lg, -1))
        rec = []
        _, _, tr = C.blocked_beam(tables, B, K, EOS, min_len, length_penalty, steps, n, ignore, record=rec)
        seqs = torch.tensor(rec[-1], dtype=torch.int64)
        # margins of this step's two top-k decisions, from the oracle alone
        lp = tables[-1].clone()
        prev = rec[-2] if t else [[] for _ in range(B * K)]
        for r, s in enumerate(prev):
            for w in (C.banned_words(s, n, ignore) if n else []):
                lp[r, w] += C.BAN_PENALTY
        if t < min_len:
            lp[:, EOS] = C.BAN_PENALTY
        kk = torch.topk(lp, K + 1).values
        if t == 0:
            cand = kk[::K]
        else:                                                             # every candidate that could enter a sample's top K
            sc = tr["scores"][:, t - 1].reshape(-1, 1) + (tr["wids"][:, t - 1].reshape(-1, 1) == EOS).float() * C.BAN_PENALTY
            cand = torch.sort((kk + sc).reshape(B, K * (K + 1)), dim=1, descending=True).values[:, :K + 1]
        margin = min(margin, float((cand[:, :-1] - cand[:, 1:]).min()))
    ids, best, tr = C.blocked_beam(tables, B, K, EOS, min_len, length_penalty, steps, n, ignore)
    return ids, best, tr, margin


def _beam_ignore_ids(P, cfg, cls, sep, feats, pos, K, steps, n):
    """ignore ids that matter: words the blocked search (no ignore set) emits often, but not its most frequent one"""
    _, _, tr, _ = oracle_blocked_beam(P, cfg, cls, sep, feats, pos, K, steps, n)
    w = tr["wids"][:, :steps].reshape(-1)
    vals, counts = torch.unique(w, return_counts=True)
    return sorted(vals[torch.argsort(counts, descending=True, stable=True)[1:3]].tolist())


# weights (oracle seeds) whose beam search repeats itself within 8 steps, so that blocking (and the ignore set) changes it -- random
# weights over a 30,522-word vocabulary seldom do; found on the CPU oracle, asserted below
@pytest.mark.parametrize("n,with_ignore,seed", [(2, False, 7), (2, True, 17), (3, False, 7), (3, True, 17)])
def test_beam_k4_blocked_matches_restatement_on_oracle_logprobs(n, with_ignore, seed):
    B, N, K, steps = 2, 8, 4, 8
    cfg, P, m, cls, sep, feats, pos = _setup("c1", B, N, seed=seed)
    ignore = _beam_ignore_ids(P, cfg, cls, sep, feats, pos, K, steps, n) if with_ignore else None
    ref_ids, ref_best, rtr, margin = oracle_blocked_beam(P, cfg, cls, sep, feats, pos, K, steps, n, ignore)
    _, _, off, _ = oracle_blocked_beam(P, cfg, cls, sep, feats, pos, K, steps, 0)
    assert not torch.equal(off["wids"], rtr["wids"])                      # blocking changes this search
    if with_ignore:
        _, _, plain, _ = oracle_blocked_beam(P, cfg, cls, sep, feats, pos, K, steps, n)
        assert not torch.equal(plain["wids"], rtr["wids"])                # ... and so does the ignore set
    print(f"oracle margin {margin:.3e}")
    ids, scores, tr = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=K, return_traces=True, no_repeat_ngram_size=n,
                                 no_repeat_ignore_ids=ignore)
    assert torch.equal(ids.cpu(), ref_ids)
    assert torch.equal(tr["wids"][:, :steps].cpu(), rtr["wids"][:, :steps])
    assert torch.equal(tr["ptrs"][:, :steps].cpu(), rtr["ptrs"][:, :steps])
    assert float((scores.cpu() - ref_best.float()).abs().max()) < 1e-3


def test_greedy_blocked_has_no_repeat_and_matches_restatement_f32_and_16bit():
    B, N, steps, n = 3, 10, GREEDY_STEPS, GREEDY_N
    cfg, P, m32, cls, sep, feats, pos = _setup("c1", B, N, seed=GREEDY_SEED)
    ref, _ = _oracle_greedy(P, cfg, cls, sep, feats, pos, steps)
    assert not bool((ref == EOS).any())
    assert any(C.has_repeated_ngram(s, n) for s in ref.tolist())          # the unblocked output does loop
    before, lp_before = m32.generate(cls, (feats, pos), sep, max_len=steps)
    assert torch.equal(before.cpu(), ref)
    ref_ids, ref_best, rtr, margin = oracle_blocked_beam(P, cfg, cls, sep, feats, pos, 1, steps, n)
    ids, scores = m32.generate(cls, (feats, pos), sep, max_len=steps, beam_size=1, no_repeat_ngram_size=n)
    assert not bool((ref_ids == EOS).any())
    assert not any(C.has_repeated_ngram(s, n) for s in ids.tolist())
    assert torch.equal(ids.cpu(), ref_ids)
    assert float((scores.cpu() - ref_best.float()).abs().max()) < 1e-3
    # the unblocked call returns what it returned before
    after, lp_after = m32.generate(cls, (feats, pos), sep, max_len=steps)
    assert torch.equal(after, before) and torch.equal(lp_after, lp_before)
    # sixteen-bit: the same words up to the first step whose oracle margin is small, as the unblocked greedy test compares
    m16 = mv.CXRBERT(_cd(cfg), None, dtype=torch.bfloat16, device=DEV)
    m16.load_state_dict(P)
    m16.eval()
    ids16, _, tr16 = m16.generate(cls, (feats, pos), sep, max_len=steps, beam_size=1, no_repeat_ngram_size=n, return_traces=True)
    w16 = tr16["wids"][:, :steps, 0].cpu()
    assert not any(C.has_repeated_ngram(s, n) for s in w16.tolist())      # whatever the rounding chose, nothing repeats
    seqs = torch.zeros((B, 0), dtype=torch.int64)
    ok = torch.ones(B, dtype=torch.bool)                                  # a sample is compared up to its first small margin
    for t in range(steps):
        lp = torch.log_softmax(_oracle_step_logits(P, cfg, cls, sep, feats, pos, seqs), -1)
        for b in range(B):
            for w in C.banned_words(seqs[b].tolist(), n):
                lp[b, w] += C.BAN_PENALTY
        top2 = torch.topk(lp, 2, dim=-1).values
        seqs = torch.cat([seqs, lp.argmax(-1, keepdim=True)], 1)
        ok &= (top2[:, 0] - top2[:, 1]) >= 2 * BF16_TOL
        assert torch.equal(w16[ok, t], seqs[ok, t]), t
    assert torch.equal(seqs, ref_ids[:, :steps])                          # (the loop above is the restated search at K = 1)


def test_blocked_batch_equals_each_sample_alone_and_training_after_generate():
    from oracle import synth
    B, N, steps, n = 3, 10, 8, 2
    cfg, P, m, cls, sep, feats, pos = _setup("c1", B, N)
    idsk, sck = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=3, no_repeat_ngram_size=n, no_repeat_ignore_ids=[1012])
    ids1, sc1 = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=1, no_repeat_ngram_size=n)
    for b in range(B):
        onek, s = m.generate(cls[b:b + 1], (feats[b:b + 1], pos[b:b + 1]), sep[b:b + 1], max_len=steps, beam_size=3, no_repeat_ngram_size=n,
                             no_repeat_ignore_ids=[1012])
        assert torch.equal(onek[0], idsk[b]) and float((s[0] - sck[b]).abs()) < 1e-4
        one1, _ = m.generate(cls[b:b + 1], (feats[b:b + 1], pos[b:b + 1]), sep[b:b + 1], max_len=steps, beam_size=1, no_repeat_ngram_size=n)
        assert torch.equal(one1[0], ids1[b])
    batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(cfg, 4, 16, 45, "mixed", seed=5).items()}
    stats = []
    for gen_first in (False, True):
        torch.manual_seed(0)
        mm = mv.CXRBERT(_cd(cfg), None, dtype=torch.bfloat16, device=DEV)
        mm.load_state_dict(P)
        mm.train()
        if gen_first:
            mm.generate(cls, (feats, pos), sep, max_len=4, beam_size=2, no_repeat_ngram_size=2)
            assert mm.training
        stats.append(mv.TrainStep(mm, lr=1e-5)(dict(batch), train=True).cpu())
    s0, s1 = stats
    assert torch.equal(s0[[1, 2, 4, 5]], s1[[1, 2, 4, 5]])                # counts and correct predictions: the same masks were drawn
    eps = torch.finfo(torch.float32).eps                                  # (the nll sums are atomic f32 sums: see test_generate_gpu.py)
    for i, cnt in ((0, 1), (3, 4)):
        assert abs(float(s0[i]) - float(s1[i])) <= float(s0[cnt]) * eps * abs(float(s0[i])), (i, float(s0[i]), float(s1[i]))


def test_switch_off_is_bit_equal_to_a_call_without_the_keyword():
    B, N, steps = 2, 8, 6
    cfg, P, m, cls, sep, feats, pos = _setup("c1", B, N)
    m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=3, no_repeat_ngram_size=2)          # a blocked call first: nothing of it may stick
    for K in (1, 3):
        a = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=K)
        b = m.generate(cls, (feats, pos), sep, max_len=steps, beam_size=K, no_repeat_ngram_size=0, no_repeat_ignore_ids=[7])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
