"""Timing of one report fine-tuning step on BERT-base at the reference's shape (B = 64, 256 regions, max_len 512 -> 254 text ids,
max_pred 10), one MI355X:
  (a) host route, f32 features      data.seq2seq_finetune_batch on the CPU, upload of the batch and of its region features as a
                                    DataLoader hands them over (f32), CXRBertForReportFinetune.forward, backward, BertAdam.step
  (b) host route, 16-bit features   the same with the host copy of the features already in the engine's input encoding
  (c) CXRBertForReportFinetune.fit_step from a data.ReportBank
The variants alternate inside one session: warm-up rounds, then `--repeats` timed rounds, each step under a host clock that ends in a
device synchronisation (the gain is host time: device events alone would hide it); median, min and max are reported.  The three
kernels of csrc/mv_report.hip are timed on their own with device events.  Writes profiles/report_bank_bench.json (and prints it).
usage: python profiles/tools/report_bank_bench.py [--batch 64] [--items 256] [--repeats 10] [--warmup 3]"""
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
from medvill_amd.data import ReportBank, seq2seq_finetune_batch  # noqa: E402

SEP = 102
N, MAX_LEN, MAX_PRED, F = 256, 512, 10, 2048
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
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_bank_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda:0"
    cd = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=512)
    model = mv.CXRBertForReportFinetune(cd, dtype=torch.bfloat16, device=dev, label_smoothing=0.1)
    model.train()
    opt = mv.optim.BertAdam(model.parameters(), lr=1e-5, weight_decay=0.01)
    n, B = a.items, a.batch
    rng = np.random.default_rng(0)
    lens = rng.integers(T // 2, T, n)                                        # raw tokens per report; the row adds the [SEP]
    raw = rng.integers(1000, 30000, (n, T)).astype(np.int64)
    rows = np.zeros((n, T), np.int64)
    for i, ln in enumerate(lens.tolist()):
        rows[i, :ln] = raw[i, :ln]
        rows[i, ln] = SEP
    feats = torch.randn((n, N, F), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(N).unsqueeze(0).repeat(n, 1)
    bank = ReportBank(model, max_pred=MAX_PRED)
    bank.add_reports(rows, lens + 1).add_images((feats, pos))
    feats16 = feats.to(bank.feat_dtype)
    raw_t, lens_t = torch.from_numpy(raw), torch.from_numpy(lens)
    gen = torch.Generator().manual_seed(2)
    state = {"step": 0}

    def batch_idx():
        state["step"] += 1
        return torch.from_numpy(np.random.default_rng(state["step"]).integers(0, n, B))

    def host_route(host_feats):
        idx = batch_idx()
        b = seq2seq_finetune_batch(raw_t[idx], lens_t[idx], N, MAX_LEN, max_pred=MAX_PRED, generator=gen)
        opt.zero_grad()
        loss, _ = model(b["cls_tok"].to(dev), b["input_txt"].to(dev), b["attn_mask"].to(dev), b["segment"].to(dev),
                        (host_feats[idx].to(dev), pos[idx].to(dev)), b["sep_tok"].to(dev), masked_lm_labels=b["masked_lm_labels"],
                        masked_pos=b["masked_pos"], masked_weights=b["masked_weights"])
        loss.backward()
        opt.step()
        return loss

    def bank_route():
        return model.fit_step(bank, batch_idx(), opt, state["step"], key=3)

    variants = (("host_route_f32_features", lambda: host_route(feats)), ("host_route_16bit_features", lambda: host_route(feats16)),
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
    res = {"config": f"bert-base B={B} N={N} T={T} max_pred={MAX_PRED} items={n}", "device": torch.cuda.get_device_name(0)}
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
        return ops.report_assemble(bank.txt_ids, bank.txt_len, bank.n_pred, bank.img_feats, bank.img_pos, idxs[turn["i"] % 16], MAX_PRED,
                                   key=3, step=turn["i"])

    out = assemble()
    vl = out["desc"][:, 2].contiguous()
    gather_bytes = 2 * B * N * F * bank.img_feats.element_size()
    k = {"mv_report_draws_ms": event_ms(lambda: ops.report_draws(3, 1, B, T, dev)),
         "mv_report_assemble_ms": event_ms(assemble),
         "mv_report_plan_ms": event_ms(lambda: ops.report_plan(out["masked_pos"], out["masked_lm_labels"], out["masked_weights"],
                                                               MAX_LEN, 30522, valid_len=vl))}
    k["bank_feature_bytes"] = bank.img_feats.numel() * bank.img_feats.element_size()
    k["assemble_gather_bytes"] = gather_bytes                                 # read + written by the feature gather
    k["assemble_gather_GBps"] = gather_bytes / (k["mv_report_assemble_ms"] * 1e-3) / 1e9
    res["kernels"] = k
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
