"""Timing of retrieval evaluation and fine-tuning on BERT-base, N = 256 regions, S = 253, groups of C = 100 candidates, one MI355X:
  evaluation, pairs/s   (a) host-built batches into CXRBertForRetrieval.score(), the image side repeated per pair (the path before
                            RetrievalBank: what a port of test(), full_dset_retrieval.py:461-510, had to do), metrics in numpy
                        (b) CXRBertForRetrieval.evaluate() from device-resident banks
  fine-tuning, steps/s  (c) forward + CrossEntropyLoss + backward + torch.optim.AdamW on host-built pair batches
                        (d) CXRBertForRetrieval.fit_step
Each variant: warm-up runs, then `--repeats` timed runs (host clock around a device synchronisation: the host work is part of what is
compared); median, min and max are reported.  mv_pair_assemble is timed on its own with device events against the bytes its feature
gather reads and writes.  Writes profiles/retrieval_bench.json (and prints it).
usage: python profiles/tools/retrieval_bench.py [--groups 4] [--batch 100] [--train-batch 16] [--repeats 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import medvill_amd as mv  # noqa: E402
from medvill_amd import hip_ops as ops  # noqa: E402
from medvill_amd.data import MaskDesc, RetrievalBank  # noqa: E402

CLS, SEP = 101, 102
N, S, C = 256, 253, 100


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=statistics.median(ts), min_s=min(ts), max_s=max(ts), runs=len(ts))


def event_ms(fn, iters=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--kernel-images", type=int, default=256, help="images of the bank mv_pair_assemble is timed over")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--train-batch", type=int, default=16, help="positives per step (the batch holds twice as many pairs)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda:0"
    cd = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=512)
    model = mv.CXRBertForRetrieval(cd, dtype=torch.bfloat16, device=dev)
    model.eval()
    G = a.groups
    rng = np.random.default_rng(0)
    # image-to-text evaluation file: group g = image g against C texts (text g * C is the aligned one)
    n_txt = G * C
    lens = rng.integers((S + 1) // 2, S + 2, n_txt).astype(np.int32)
    ids = np.zeros((n_txt, S + 1), dtype=np.int64)
    for i, l in enumerate(lens.tolist()):
        ids[i, :l - 1] = rng.integers(1000, 30000, l - 1)
        ids[i, l - 1] = SEP
    feats = torch.randn((G, N, 2048), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(N).unsqueeze(0).repeat(G, 1)
    pairs = torch.tensor([(g, g * C + c) for g in range(G) for c in range(C)], dtype=torch.int32)
    labels = torch.tensor([1 if c == 0 else 0 for g in range(G) for c in range(C)], dtype=torch.int32)
    bank = RetrievalBank(model)
    bank.add_texts(ids, lens).add_images((feats, pos))
    ids_t, lens_t = torch.from_numpy(ids), torch.from_numpy(lens)

    def host_batch(p):
        im, tx = p[:, 0].long(), p[:, 1].long()
        R = p.shape[0]
        return (torch.full((R, 1), CLS), ids_t[tx], MaskDesc.make("1d", N, S, lens_t[tx], dev), torch.ones((R, S + 1), dtype=torch.int64),
                (feats[im], pos[im]), torch.full((R, 1), SEP))

    def eval_before():
        out = []
        for s in range(0, pairs.shape[0], a.batch):
            out.append(model.score(*host_batch(pairs[s:s + a.batch])))
        p = torch.cat(out).cpu().numpy().reshape(G, C)
        lab = labels.numpy().reshape(G, C)
        ranks = [int(np.flatnonzero(lab[g][np.argsort(p[g], kind="stable")[::-1]] == 1)[0]) for g in range(G)]
        return float(np.mean([1.0 / (r + 1) for r in ranks]))

    def eval_banks():
        return model.evaluate(bank, pairs, labels, group_size=C, batch_size=a.batch)["mrr_score"]

    res = {"config": f"bert-base N={N} S={S} C={C}", "groups": G, "pairs": int(pairs.shape[0]), "eval_batch": a.batch,
           "train_pairs_per_step": 2 * a.train_batch, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("eval_score_host_batches", eval_before), ("eval_evaluate_from_banks", eval_banks)):
        t = timed(fn, a.warmup, a.repeats)
        t["pairs_per_s"] = pairs.shape[0] / t["median_s"]
        res[name] = t
        print(name, json.dumps(t), file=sys.stderr, flush=True)
    res["eval_speedup"] = res["eval_score_host_batches"]["median_s"] / res["eval_evaluate_from_banks"]["median_s"]

    # fine-tuning: a data set of n items (image i, text i)
    n = G
    tb = RetrievalBank(model)
    tb.add_texts(ids[::C][:n], lens[::C][:n]).add_images((feats, pos))
    B = min(a.train_batch, n)
    idx = torch.arange(B, dtype=torch.int32)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5, eps=1e-6, weight_decay=0.0)
    crit = torch.nn.CrossEntropyLoss()
    sub_ids, sub_lens = ids_t[::C][:n], lens_t[::C][:n]
    state = {"step": 0}

    def train_before():
        state["step"] += 1
        r = torch.randint(0, n - 1, (B,))
        other = r + (r >= idx).long()
        coin = torch.rand(B) > 0.5
        im = torch.cat([idx.long(), torch.where(coin, other, idx.long())])
        tx = torch.cat([idx.long(), torch.where(coin, idx.long(), other)])
        lab = torch.cat([torch.ones(B), torch.zeros(B)]).long().to(dev)
        R = 2 * B
        logits = model(torch.full((R, 1), CLS), sub_ids[tx], MaskDesc.make("1d", N, S, sub_lens[tx], dev),
                       torch.ones((R, S + 1), dtype=torch.int64), (feats[im], pos[im]), torch.full((R, 1), SEP))
        loss = crit(logits.view(-1, 2), lab.view(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()                     # the reference reads the loss every step (:387)

    def train_fit():
        state["step"] += 1
        return model.fit_step(tb, idx, 1e-5, state["step"], key=1)

    for name, fn in (("train_forward_ce_backward_torch_adamw", train_before), ("train_fit_step", train_fit)):
        state["step"] = 0
        t = timed(fn, a.warmup, a.repeats)
        t["steps_per_s"] = 1.0 / t["median_s"]
        res[name] = t
        print(name, json.dumps(t), file=sys.stderr, flush=True)
    res["train_speedup"] = res["train_forward_ce_backward_torch_adamw"]["median_s"] / res["train_fit_step"]["median_s"]

    # mv_pair_assemble on its own at the banks' benchmark configuration (R = 64 pairs, 16-bit features), device events (launch after
    # launch, the wrapper's allocations included).  The pairs rotate over a bank of --kernel-images images: with a bank larger than
    # the 256 MiB Infinity Cache the gathered rows come from HBM, as they do in an epoch
    R, n_k = 64, a.kernel_images
    kb = RetrievalBank(model)
    kb.add_texts(ids[:n_k], lens[:n_k]).add_images((torch.randn((n_k, N, 2048), generator=torch.Generator().manual_seed(2)),
                                                    torch.arange(N).unsqueeze(0).repeat(n_k, 1)))
    kp = [torch.from_numpy(np.stack([rng.integers(0, n_k, R), rng.integers(0, kb.n_texts, R)], 1).astype(np.int32)).to(dev)
          for _ in range(16)]
    turn = {"i": 0}

    def assemble():
        turn["i"] += 1
        return ops.pair_assemble(kb.txt_ids, kb.txt_len, kb.img_feats, kb.img_pos, kp[turn["i"] % 16])

    gather_bytes = 2 * R * N * 2048 * kb.img_feats.element_size()
    k = {"mv_pair_assemble_ms": event_ms(assemble), "bank_feature_bytes": kb.img_feats.numel() * kb.img_feats.element_size(),
         "assemble_gather_bytes": gather_bytes}                                # read + written by the feature gather
    k["assemble_gather_GBps"] = gather_bytes / (k["mv_pair_assemble_ms"] * 1e-3) / 1e9
    res["kernels"] = k
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
