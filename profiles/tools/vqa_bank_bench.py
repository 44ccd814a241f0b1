"""Timing of one VQA fine-tuning step on BERT-base at the reference's shape (B = 64, 256 regions, max_len 512 -> 254 text ids, 458
answers) over a data set of VQA-RAD's size (315 images, 3,064 questions), one MI355X:
  (a) host route, 16-bit features   the batch built per step on the CPU as the reference's loader does (question rows, segment, mask
                                    descriptors, the dense soft target by scatter_, answer types), upload of the batch and of the
                                    region features of each question's image from a host copy already in the engine's input encoding,
                                    CXRBertForVQA.forward, backward, BertAdam.step
  (b) host route, f32 features      the same with the features as a DataLoader hands them over (f32)
  (c) CXRBertForVQA.fit_step from a data.VqaBank
The variants alternate inside one session: warm-up rounds, then `--repeats` timed rounds, each step under a host clock that ends in a
device synchronisation (the gain is host time: device events alone would hide it); median, min and max are reported.  mv_vqa_assemble
is timed on its own with device events against the bytes its feature gather reads and writes, and mv_vqa_score over one batch.  Writes
profiles/vqa_bank_bench.json (and prints it).
usage: python profiles/tools/vqa_bank_bench.py [--batch 64] [--images 315] [--questions 3064] [--repeats 10] [--warmup 3]"""
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
from medvill_amd.data import MaskDesc, VqaBank  # noqa: E402

SEP = 102
N, MAX_LEN, F, A = 256, 512, 2048, 458
T = MAX_LEN - N - 2


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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--images", type=int, default=315)
    ap.add_argument("--questions", type=int, default=3064)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vqa_bank_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda:0"
    cd = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=512)
    model = mv.CXRBertForVQA(cd, dtype=torch.bfloat16, device=dev, n_answers=A)
    model.train()
    opt = mv.optim.BertAdam(model.parameters(), lr=1e-5, weight_decay=0.01)
    n_img, n, B = a.images, a.questions, a.batch
    rng = np.random.default_rng(0)
    lens = rng.integers(4, 24, n)                                            # question tokens; the row adds the [SEP]
    rows = np.zeros((n, T), np.int64)
    for i, ln in enumerate(lens.tolist()):
        rows[i, :ln] = rng.integers(1000, 30000, ln)
        rows[i, ln] = SEP
    q_img = rng.integers(0, n_img, n)
    labels = [rng.integers(0, A, int(k)).tolist() for k in rng.integers(0, 4, n)]
    scores = [[1.0, 0.6, 0.3][:len(l)] for l in labels]
    types = rng.integers(0, 2, n).tolist()
    feats = torch.randn((n_img, N, F), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(N).unsqueeze(0).repeat(n_img, 1)
    bank = VqaBank(model, n_answers=A)
    bank.add_images((feats, pos)).add_questions(rows, lens + 1, q_img, labels, scores, types)
    feats16 = feats.to(bank.feat_dtype)
    rows_t, q_img_t = torch.from_numpy(rows), torch.from_numpy(q_img)
    state = {"step": 0}

    def batch_idx():
        state["step"] += 1
        return torch.from_numpy(np.random.default_rng(state["step"]).integers(0, n, B))

    def host_route(host_feats):
        idx = batch_idx()
        il = idx.tolist()
        n_ids = torch.from_numpy(lens[il] + 1)
        segment = (torch.arange(T).view(1, T) < n_ids.view(B, 1)).to(torch.int64)
        target = torch.zeros((B, A))
        for b, q in enumerate(il):                                           # data_loader.py:269-271
            if labels[q]:
                target[b].scatter_(0, torch.tensor(labels[q]), torch.tensor(scores[q]))
        ans_type = torch.tensor([types[q] for q in il], dtype=torch.int32)
        im = q_img_t[idx]
        opt.zero_grad()
        _, loss = model(torch.full((B, 1), 101).to(dev), rows_t[idx].to(dev), MaskDesc.make("1d", N, T - 1, n_ids, dev), segment.to(dev),
                        (host_feats[im].to(dev), pos[im].to(dev)), torch.full((B, 1), SEP).to(dev), ans_labels=target, ans_type=ans_type)
        loss.backward()
        opt.step()
        return loss

    def bank_route():
        return model.fit_step(bank, batch_idx(), opt)

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
    res = {"config": f"bert-base B={B} N={N} T={T} A={A} images={n_img} questions={n}", "device": torch.cuda.get_device_name(0)}
    for name, v in ts.items():
        res[name] = dict(median_ms=1e3 * statistics.median(v), min_ms=1e3 * min(v), max_ms=1e3 * max(v), runs=len(v))
    for name in ("host_route_f32_features", "host_route_16bit_features"):
        res[name + "_over_fit_step"] = res[name]["median_ms"] / res["fit_step_from_bank"]["median_ms"]

    # the kernels on their own, device events (launch after launch, the wrappers' allocations included).  The batches rotate over the
    # bank: with a bank larger than the 256 MiB Infinity Cache the gathered rows come from HBM, as they do in an epoch
    idxs = [torch.from_numpy(rng.integers(0, n, B).astype(np.int32)).to(dev) for _ in range(16)]
    turn = {"i": 0}

    def assemble():
        turn["i"] += 1
        return ops.vqa_assemble(bank.txt_ids, bank.txt_len, bank.q_img, bank.ans_ptr, bank.ans_label, bank.ans_score, bank.ans_type,
                                bank.img_feats, bank.img_pos, idxs[turn["i"] % 16], A)

    pred = torch.from_numpy(rng.integers(0, A, B)).to(dev)
    counters = torch.zeros((8, 3, 2), dtype=torch.int64, device=dev)
    gather_bytes = 2 * B * N * F * bank.img_feats.element_size()
    k = {"mv_vqa_assemble_ms": event_ms(assemble),
         "mv_vqa_score_ms": event_ms(lambda: ops.vqa_score(pred, idxs[0], bank.ans_ptr, bank.ans_label, bank.ans_score, bank.ans_type,
                                                           group=bank.group, counters=counters))}
    k["bank_feature_bytes"] = bank.img_feats.numel() * bank.img_feats.element_size()
    k["assemble_gather_bytes"] = gather_bytes                                 # read + written by the feature gather
    k["assemble_gather_GBps"] = gather_bytes / (k["mv_vqa_assemble_ms"] * 1e-3) / 1e9
    res["kernels"] = k
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
