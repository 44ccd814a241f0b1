"""Timing of VQA fine-tuning and answer prediction (CXRBertForVQA) at BERT-base, N = 256 regions, L = 512, A = 458 answers.

  step      ms per fine-tuning step: forward (ans_labels), loss, backward, medvill_amd.optim.AdamW -- the s2s mask (the fine-tuning
            pipeline's default) and the full (bi) mask, B in {32, 64}, after a warm-up, host clock around synchronised steps
  baseline  the route this feature replaces, on the same model: model.bert.enc(...) -> [B, L, H], a torch Linear-ReLU-Linear head on
            [:, 0], BCEWithLogitsLoss, backward through the encoder, torch.optim.AdamW over every parameter
  infer     questions / s of forward(..., vqa_inference=True) under torch.no_grad()
usage: python profiles/tools/vqa_bench.py [--batches 32,64] [--steps 10] [--warmup 3] [--out FILE] -> one JSON line"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import medvill_amd as mv  # noqa: E402
from oracle import data_oracle as D  # noqa: E402

N, S, A = 256, 253, 458


def batch(B, family, seed):
    g = torch.Generator().manual_seed(seed)
    T = S + 1
    ids = torch.zeros((B, T), dtype=torch.int64)
    masks = []
    for b in range(B):
        n = int(torch.randint(S // 4, S, (1,), generator=g))
        ids[b, :n] = torch.randint(1000, 30522, (n,), generator=g)
        ids[b, n] = 102
        masks.append(torch.from_numpy(D.build_mask(family, N, S, n + 1)))
    t = torch.zeros(B, A)
    t[torch.arange(B), torch.randint(0, A, (B,), generator=g)] = 1.0
    dev = "cuda:0"
    return dict(args=(torch.full((B, 1), 101, device=dev), ids.to(dev), torch.stack(masks).to(dev), torch.zeros_like(ids).to(dev),
                      (torch.randn((B, N, 2048), generator=g).to(dev), torch.sort(torch.randperm(256, generator=g)[:N]).values.repeat(B, 1).to(dev)),
                      torch.full((B, 1), 102, device=dev)),
                target=t.to(dev), ans_type=(torch.arange(B) % 2).to(dev))


def timeit(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,64")
    ap.add_argument("--families", default="s2s,full")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    cd = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=512)
    model = mv.CXRBertForVQA(cd, dtype=torch.bfloat16, device="cuda:0")
    model.train()
    opt = mv.optim.AdamW(model.parameters(), lr=1e-5)
    H = 768
    # baseline head: plain torch modules on the same device (their own weights: the time, not the values, is compared)
    head = nn.Sequential(nn.Linear(H, 2 * H), nn.ReLU(), nn.Linear(2 * H, A)).cuda()
    res = {"config": "bert-base N=256 L=512 A=458 bf16 (f16 operands)", "steps": a.steps, "warmup": a.warmup, "runs": []}
    for family in a.families.split(","):
        for B in [int(x) for x in a.batches.split(",")]:
            bt = batch(B, family, seed=B)

            def step():
                opt.zero_grad()
                _, loss = model(*bt["args"], ans_labels=bt["target"], ans_type=bt["ans_type"])
                loss.backward()
                opt.step()
                return loss

            ms = timeit(step, a.steps, a.warmup)
            loss = float(step())
            base_opt = torch.optim.AdamW(list(model.parameters()) + list(head.parameters()), lr=1e-5)

            def base_step():
                base_opt.zero_grad()
                hid, _, _ = model.bert.enc(*bt["args"])
                loss_ = F.binary_cross_entropy_with_logits(head(hid[:, 0].float()), bt["target"])
                loss_.backward()
                base_opt.step()

            base_ms = timeit(base_step, a.steps, a.warmup)
            del base_opt
            model.eval()
            with torch.no_grad():
                inf_ms = timeit(lambda: model(*bt["args"], vqa_inference=True), a.steps, a.warmup)
            model.train()
            res["runs"].append(dict(family=family, B=B, step_ms=round(ms, 3), baseline_step_ms=round(base_ms, 3),
                                    speedup=round(base_ms / ms, 3), infer_ms=round(inf_ms, 3), infer_questions_per_s=round(B * 1e3 / inf_ms, 1),
                                    loss=round(loss, 6)))
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
