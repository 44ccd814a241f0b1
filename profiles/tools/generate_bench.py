"""Timing of KV-cached report generation (CXRBERT.generate) on BERT-base, N = 180 regions, max_len 254: prefill and per-token decode at
B in {1, 8, 64} x beam {1, 4}, after a warm-up, with HIP events; achieved bandwidth against the byte model of DESIGN.md "Generation";
and, as the baseline, the same greedy generation by one full CXRBERT.forward per step (s2s mask, every step recomputed).
--no-repeat-ngram n times the same decode steps once more with n-gram blocking on: every step followed by the history /
ban-list update (mv_ngram_ban) and read through mv_logprob_topk_banned, on histories of a few words (so that every beam has bans);
--repeats r times every loop r times, so that the spread of the unblocked step is known before the two are compared.
usage: python profiles/tools/generate_bench.py [--batches 1,8,64] [--beams 1,4] [--max-len 254] [--recompute-steps 16]
       [--no-repeat-ngram 3 --repeats 5] -> one JSON line"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import medvill_amd as mv  # noqa: E402
from medvill_amd.generate import Generator  # noqa: E402

CLS, SEP, MASK = 101, 102, 103


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--beams", default="1,4")
    ap.add_argument("--max-len", type=int, default=254)
    ap.add_argument("--steps", type=int, default=32, help="decode steps timed per configuration (after 4 warm-up steps)")
    ap.add_argument("--recompute-steps", type=int, default=16)
    ap.add_argument("--no-repeat-ngram", type=int, default=0, help="also time the decode steps with n-gram blocking of this size")
    ap.add_argument("--repeats", type=int, default=1, help="timed repetitions of every decode loop")
    a = ap.parse_args()
    torch.manual_seed(0)
    cd = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=512)
    model = mv.CXRBERT(cd, None, dtype=torch.bfloat16, device="cuda:0")
    model.eval()
    eng, cfg = model.engine, model.cfg
    N, H = 180, cfg.hidden
    # byte model: the 16-bit weights one decode step streams (12 layers + MLM transform + tied decoder) and the K/V it reads
    wbytes = 2 * (cfg.layers * (4 * H * H + 2 * H * cfg.intermediate) + H * H + cfg.vocab_size * H)
    res = {"config": "bert-base N=180", "max_len": a.max_len, "weights_MB_per_step": wbytes / 1e6, "runs": []}
    for B in [int(x) for x in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        feats = torch.randn((B, N, 2048), generator=g)
        pos = torch.sort(torch.randperm(256, generator=g)[:N]).values.unsqueeze(0).repeat(B, 1)
        cls = torch.full((B, 1), CLS, dtype=torch.int64)
        sep = torch.full((B, 1), SEP, dtype=torch.int64)
        for K in [int(x) for x in a.beams.split(",")]:
            gen = Generator(eng)
            prev = (eng.training, eng.keep_acts)
            eng.training, eng.keep_acts = False, True
            with torch.no_grad():
                gen._alloc(B, N, K, a.max_len)
                for _ in range(2):
                    t_pre, _ = timed(lambda: gen.prefill(cls, feats, pos, sep, MASK))
                y = torch.full((B * K,), 1000, dtype=torch.int64, device=eng.device)
                for t in range(4):
                    gen.step(t, y, MASK, K, -1)
                # steady decode steps at the mean history length of a 254-token report (t around max_len / 2)
                t0 = a.max_len // 2
                torch.cuda.synchronize()
                reps = [timed(lambda: [gen.step(t0 + i, y, MASK, K, -1) for i in range(a.steps)])[0] / a.steps for _ in range(a.repeats)]
                blocked = []
                if a.no_repeat_ngram:
                    gen.ngram_on(a.no_repeat_ngram, [])
                    words = torch.randint(1000, 1012, (B * K, a.max_len), generator=g).to(torch.int32).to(eng.device)
                    gen.hist[0].copy_(words)
                    gen.hist[1].copy_(words)
                    parents = torch.arange(B * K, dtype=torch.int64, device=eng.device)

                    def blocked_steps():
                        for i in range(a.steps):
                            gen.step(t0 + i, y, MASK, K, -1)
                            gen.ngram_update(t0 + i, parents, y)
                    blocked_steps()
                    torch.cuda.synchronize()
                    blocked = [timed(blocked_steps)[0] / a.steps for _ in range(a.repeats)]
                    nban_mean = float(gen.nban.float().mean())
                    gen.ngram = 0
            eng.training, eng.keep_acts = prev
            per = sorted(reps)[len(reps) // 2]
            keys = N + 2 + t0
            kv_bytes = 2 * B * K * keys * 2 * H * cfg.layers * 2          # two rows per beam, K and V, 16-bit
            run = {"B": B, "beam": K, "prefill_ms": t_pre, "decode_ms_per_token": per, "tokens_per_s": B * 1e3 / per,
                   "mean_keys": keys, "achieved_GBps": (wbytes + kv_bytes) / (per * 1e-3) / 1e9,
                   "modelled_ms_per_token": (wbytes + kv_bytes) / 6e12 * 1e3}
            if a.repeats > 1:
                run["decode_ms_per_token_repeats"] = reps
            if blocked:
                run.update(no_repeat_ngram=a.no_repeat_ngram, blocked_ms_per_token=sorted(blocked)[len(blocked) // 2],
                           blocked_ms_per_token_repeats=blocked, mean_banned_words=nban_mean)
            if K == 1 and a.recompute_steps > 0:
                # baseline: greedy by full forward recompute, s2s mask over the whole prefix + text so far, every step
                def recompute():
                    txt = torch.zeros((B, 0), dtype=torch.int64)
                    with torch.no_grad():
                        for t in range(a.recompute_steps):
                            tt = torch.cat([txt, torch.full((B, 1), MASK, dtype=torch.int64)], 1)
                            T, L = tt.shape[1], N + 2 + tt.shape[1]
                            m = torch.zeros((B, L, L), dtype=torch.int64)
                            m[:, :, :N + 2] = 1
                            m[:, N + 2:, N + 2:] = torch.tril(torch.ones((T, T), dtype=torch.int64))
                            mlm, _ = model(cls, tt, m.cuda(), torch.ones_like(tt), (feats, pos), sep)
                            txt = torch.cat([txt, mlm[:, N + 2 + t].argmax(-1, keepdim=True).cpu()], 1)
                recompute()
                rms, _ = timed(recompute)
                # the cached path over the same steps (prefill + decode), for the speed-up
                cms, _ = timed(lambda: model.generate(cls, (feats, pos), sep, max_len=a.recompute_steps))
                run.update(recompute_ms_first_steps=rms, cached_ms_first_steps=cms, speedup_vs_recompute=rms / cms,
                           recompute_steps=a.recompute_steps)
            res["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
