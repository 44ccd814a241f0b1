"""Timing of one diagnosis-classification fine-tuning step on BERT-base at the reference's shape (B = 64, 256 regions, max_len 512 ->
254 text ids, 14 classes) over a data set of 3,000 samples on 600 images, one MI355X:
  (a) host route, 16-bit features   the batch built per step on the CPU as the reference's JsonlDataset + collate_fn do (text rows,
                                    segment, mask descriptors, the multi-hot target), upload of the batch and of the region features of
                                    each sample's image from a host copy already in the engine's input encoding,
                                    CXRBertForClassification.forward(labels=), backward, BertAdam.step
  (b) host route, f32 features      the same with the features as a DataLoader hands them over (f32)
  (c) CXRBertForClassification.fit_step from a data.ClassificationBank
The variants alternate inside one session: warm-up rounds, then `--repeats` timed rounds, each step under a host clock that ends in a
device synchronisation (the gain is host time: device events alone would hide it); median, min and max are reported.  mv_clf_assemble
is timed on its own with device events against the bytes its feature gather reads and writes, before the training rounds and again
after them.  mv_clf_counts is timed with device
events at n = 4096, C = 14 and at its limit n C = 2^21 (n = 149796, C = 14), on sigmoid probabilities with 30 % saturated to 0 / 1 and
labels set with probability 0.1, beside classification.metrics() on the host over the same probabilities (host clock, the copy to the
host included).  Writes profiles/clf_bank_bench.json (and prints it).
usage: python profiles/tools/clf_bank_bench.py [--batch 64] [--images 600] [--samples 3000] [--repeats 10] [--warmup 3]"""
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
from medvill_amd import classification  # noqa: E402
from medvill_amd import hip_ops as ops  # noqa: E402
from medvill_amd.data import ClassificationBank, MaskDesc  # noqa: E402

SEP = 102
N, MAX_LEN, F, C = 256, 512, 2048, 14
T = MAX_LEN - N - 2


def event_ms(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def counts_against_host(n, dev, iters, host_runs):
    """mv_clf_counts (device events) and classification.metrics (host clock) over the same n x C probabilities."""
    g = torch.Generator().manual_seed(n)
    probs = torch.sigmoid(3.0 * torch.randn((n, C), generator=g))
    u = torch.rand((n, C), generator=g)
    probs = torch.where(u < 0.15, torch.zeros(()), torch.where(u < 0.3, torch.ones(()), probs))
    hot = torch.rand((n, C), generator=g) < 0.1
    bank = ClassificationBank(device=dev, n_classes=C)
    bank.add_samples(torch.zeros((n, 2), dtype=torch.int64), [1] * n, hot)
    probs_d, idx = probs.to(dev), torch.arange(n, dtype=torch.int32, device=dev)
    counters = torch.zeros((C + 1, ops.CLF_NCOUNT), dtype=torch.int64, device=dev)
    ms = event_ms(lambda: ops.clf_counts(probs_d, idx, bank.lab_bits, C, counters=counters), iters=iters, warm=2)
    got = classification.metrics_from_counters(ops.clf_counts(probs_d, idx, bank.lab_bits, C))
    target = bank.dense_targets(torch.arange(n))
    host = []
    for _ in range(host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = classification.metrics(probs_d, target)
        host.append(1e3 * (time.perf_counter() - t0))
    return dict(n=n, C=C, mv_clf_counts_ms=ms, host_metrics_ms=statistics.median(host), host_runs=host_runs,
                equal_to_host_metrics=all(got[k] == want[k] for k in want), micro_auroc=got["micro_auroc"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--images", type=int, default=600)
    ap.add_argument("--samples", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clf_bank_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda:0"
    cd = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=512)
    model = mv.CXRBertForClassification(cd, dtype=torch.bfloat16, device=dev, n_classes=C)
    model.train()
    opt = mv.optim.BertAdam(model.parameters(), lr=1e-5, weight_decay=0.01)
    n_img, n, B = a.images, a.samples, a.batch
    rng = np.random.default_rng(0)
    lens = rng.integers(20, 120, n)                                          # report tokens; the row adds the [SEP]
    rows = np.zeros((n, T), np.int64)
    for i, ln in enumerate(lens.tolist()):
        rows[i, :ln] = rng.integers(1000, 30000, ln)
        rows[i, ln] = SEP
    hot = torch.from_numpy(rng.random((n, C)) < 0.1)
    hot[0], hot[1] = True, False
    s_img = rng.integers(0, n_img, n)
    feats = torch.randn((n_img, N, F), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(N).unsqueeze(0).repeat(n_img, 1)
    bank = ClassificationBank(model, n_classes=C)
    bank.add_images((feats, pos)).add_samples(rows, lens + 1, hot, image_item=s_img)
    model.set_pos_weight(bank.pos_weight())
    feats16 = feats.to(bank.feat_dtype)
    rows_t, hot_f, s_img_t = torch.from_numpy(rows), hot.to(torch.float32), torch.from_numpy(s_img)
    state = {"step": 0}

    def batch_idx():
        state["step"] += 1
        return torch.from_numpy(np.random.default_rng(state["step"]).integers(0, n, B))

    def host_route(host_feats):
        idx = batch_idx()
        n_ids = torch.from_numpy(lens[idx.tolist()] + 1)
        segment = (torch.arange(T).view(1, T) < n_ids.view(B, 1)).to(torch.int64)
        im = s_img_t[idx]
        opt.zero_grad()
        loss = model(torch.full((B, 1), 101).to(dev), rows_t[idx].to(dev), MaskDesc.make("1d", N, T - 1, n_ids, dev), segment.to(dev),
                     (host_feats[im].to(dev), pos[im].to(dev)), torch.full((B, 1), SEP).to(dev), labels=hot_f[idx])
        loss.backward()
        opt.step()
        return loss

    def bank_route():
        return model.fit_step(bank, batch_idx(), opt)

    # the assemble kernel on its own, device events (launch after launch, the wrapper's allocations included).  The batches rotate
    # over the bank: it is larger than the 256 MiB Infinity Cache, so the gathered rows come from HBM, as they do in an epoch
    idxs = [torch.from_numpy(rng.integers(0, n, B).astype(np.int32)).to(dev) for _ in range(16)]
    turn = {"i": 0}

    def assemble():
        turn["i"] += 1
        return ops.clf_assemble(bank.txt_ids, bank.txt_len, bank.s_img, bank.lab_bits, bank.img_feats, bank.img_pos, idxs[turn["i"] % 16], C)

    assemble_first_ms = event_ms(assemble)                                    # before any training step of this process

    variants = (("host_route_16bit_features", lambda: host_route(feats16)), ("host_route_f32_features", lambda: host_route(feats)),
                ("fit_step_from_bank", bank_route))
    ts = {name: [] for name, _ in variants}
    for r in range(a.warmup + a.repeats):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ts[name].append(time.perf_counter() - t0)
    res = {"config": f"bert-base B={B} N={N} T={T} C={C} images={n_img} samples={n}", "device": torch.cuda.get_device_name(0)}
    for name, v in ts.items():
        res[name] = dict(median_ms=1e3 * statistics.median(v), min_ms=1e3 * min(v), max_ms=1e3 * max(v), runs=len(v))
    for name in ("host_route_f32_features", "host_route_16bit_features"):
        res[name + "_over_fit_step"] = res[name]["median_ms"] / res["fit_step_from_bank"]["median_ms"]

    gather_bytes = 2 * B * N * F * bank.img_feats.element_size()
    k = {"mv_clf_assemble_ms": assemble_first_ms, "mv_clf_assemble_after_training_ms": event_ms(assemble)}
    k["bank_feature_bytes"] = bank.img_feats.numel() * bank.img_feats.element_size()
    k["assemble_gather_bytes"] = gather_bytes                                 # read + written by the feature gather
    k["assemble_gather_GBps"] = gather_bytes / (k["mv_clf_assemble_ms"] * 1e-3) / 1e9
    res["kernels"] = k
    res["counts"] = [counts_against_host(4096, dev, iters=50, host_runs=5),
                     counts_against_host(ops.CLF_MAX_ELEMS // C, dev, iters=3, host_runs=2)]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
