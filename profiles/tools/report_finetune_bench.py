"""Time one report fine-tuning step of CXRBertForReportFinetune against the route the package offered before it: `lazy_logits` +
`losses.mlm_itm_loss(itm_task=False)` + the same optimizer (a plain mean cross-entropy over the labelled rows: no smoothing, no
weights, no drop-worst -- a different objective, timed as the closest existing step).  BERT-base, B=64, L=512, max_pred=10, f16 path.

    python profiles/tools/report_finetune_bench.py [--steps 20] [--warmup 5] [--out profiles/report_finetune_bench.json]

Device events around each step (forward, backward, optimizer) after warm-up steps; the median, minimum and maximum over the timed steps
are reported.  The batch comes from data.seq2seq_finetune_batch (host), moved to the device once."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import medvill_amd as mv                     # noqa: E402
from medvill_amd import losses               # noqa: E402

CFG = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
           max_position_embeddings=512)


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "report_finetune_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    B, N, L, max_pred = a.batch, 256, 512, 10
    T = L - N - 2
    g = torch.Generator().manual_seed(0)
    lengths = torch.randint((T - 1) // 2, T, (B,), generator=g)
    ids = torch.randint(1000, CFG["vocab_size"], (B, T - 1), generator=g)
    b = mv.data.seq2seq_finetune_batch(ids, lengths, N, L, max_pred=max_pred, generator=g)
    feats = torch.randn(B, N, 2048, generator=g).to(dev, torch.float16)
    pos = torch.arange(N).view(1, N).expand(B, N).contiguous().to(dev)
    inputs = (b["cls_tok"].to(dev), b["input_txt"].to(dev), b["attn_mask"].to(dev), b["segment"].to(dev), (feats, pos), b["sep_tok"].to(dev))
    lists = dict(masked_lm_labels=b["masked_lm_labels"], masked_pos=b["masked_pos"], masked_weights=b["masked_weights"])
    # the lazy route's labels: one label per DISTINCT listed position (it cannot express a position listed twice)
    labels = torch.full((B, L), -100, dtype=torch.int64)
    on = b["masked_weights"] > 0
    for s in range(B):
        labels[s, b["masked_pos"][s][on[s]]] = b["masked_lm_labels"][s][on[s]]
    labels, aligned = labels.to(dev), torch.ones(B, dtype=torch.int64, device=dev)
    res = dict(config=dict(B=B, L=L, N=N, max_pred=max_pred, path="f16", label_smoothing=0.1, drop_worst_ratio=0.0),
               device=torch.cuda.get_device_name(0))

    torch.manual_seed(0)
    m = mv.CXRBertForReportFinetune(CFG, dtype=torch.bfloat16, device=dev, label_smoothing=0.1)
    m.train()
    opt = mv.optim.BertAdam(m.parameters(), lr=3e-5, weight_decay=0.01)

    def step_new():
        opt.zero_grad()
        loss, _ = m(*inputs, **lists, drop_worst_ratio=0.0)
        loss.backward()
        opt.step()
    res["report_finetune"] = timed(step_new, a.steps, a.warmup)
    res["report_finetune"]["distinct_rows"] = int(m.bert.engine.S["n_lab"])
    del m, opt
    torch.cuda.empty_cache()

    torch.manual_seed(0)
    bert = mv.CXRBERT(CFG, dtype=torch.bfloat16, device=dev)
    bert.lazy_logits = True
    bert.train()
    opt = mv.optim.BertAdam(bert.parameters(), lr=3e-5, weight_decay=0.01)

    def step_old():
        opt.zero_grad()
        mlm, itm = bert(*inputs, txt_labels=labels)
        loss = losses.mlm_itm_loss(mlm, itm, labels, aligned, itm_task=False)
        loss.backward()
        opt.step()
    res["lazy_logits_route"] = timed(step_old, a.steps, a.warmup)
    res["ratio_new_over_old"] = res["report_finetune"]["median_ms"] / res["lazy_logits_route"]["median_ms"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
