"""Timing of the BLEU stage of a report-generation evaluation on one MI355X: n = 4096 generated rows of 128 tokens, scored against
128-word references, over a synthetic vocabulary of 30,522 tokens of which every fourth is a '##' continuation.
  (a) mv_bleu_words + mv_bleu_counts   the two launches (hip_ops.bleu_words, bleu_counts, the wrappers' allocations included), device
                                       events around `--iters` back-to-back pairs after warm-up pairs
  (b) the string reference in Python   tests/bleu_cases.py's hyp_words + string_counts (detokenize, join / split, collections.Counter)
                                       over the same ids, host clock, the copy of the ids to the host included
Token and word ids follow a Zipf-like law, so that rows repeat words and share them with their references.  The counters of (a) and (b)
are compared.  Writes profiles/bleu_bench.json (and prints it).
usage: python profiles/tools/bleu_bench.py [--n 4096] [--tokens 128] [--iters 200] [--host-runs 3] [--out PATH]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import medvill_amd  # noqa: E402,F401
from medvill_amd import hip_ops as ops  # noqa: E402
from medvill_amd import report_eval as RE  # noqa: E402
import bleu_cases as C  # noqa: E402

V, FIRST = 30522, 1000


def vocabulary():
    tokens = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    tokens += [f"[unused{i}]" for i in range(99, 99 + FIRST - len(tokens))]
    tokens += [("##p%d" if i % 4 == 3 else "w%d") % i for i in range(FIRST, V)]
    return tokens


def zipf_ids(g, shape):
    """ids in [FIRST, V) with weight ~ 1 / rank."""
    r = np.exp(g.random(shape) * np.log(V - FIRST)).astype(np.int64)
    return FIRST + np.minimum(r, V - FIRST) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bleu_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    tokens = vocabulary()
    tb = RE.word_tables(tokens)
    tok_key, tail_key, tail_pow = (tb[k].to(dev) for k in ("tok_key", "tail_key", "tail_pow"))
    sep_id, pad_id = tokens.index("[SEP]"), tokens.index("[PAD]")
    g = np.random.default_rng(0)
    ids = zipf_ids(g, (a.n, a.tokens))
    ref_ids = zipf_ids(g, (a.n, a.tokens))
    ref_ids -= ref_ids % 4 == 3                                                 # whole words only
    copy = g.random((a.n, a.tokens)) < 0.3                                      # a third of the reference repeats the row's start tokens
    ref_ids = np.where(copy & (ids % 4 != 3), ids, ref_ids)
    refs = [" ".join(tokens[i] for i in row) for row in ref_ids]
    rk, rn = RE.text_keys(refs)
    rk, rn = rk.to(dev), rn.to(dev)
    ids_d = torch.from_numpy(ids).to(dev)
    idx = torch.arange(a.n, dtype=torch.int32, device=dev)

    def launches(counters=None):
        hk, hn = ops.bleu_words(ids_d, tok_key, tail_key, tail_pow, sep_id, pad_id, tb["empty_key"])
        return ops.bleu_counts(hk, hn, rk, rn, idx, counters=counters)

    for _ in range(5):
        launches()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sink = torch.zeros(ops.BLEU_NCOUNT, dtype=torch.int64, device=dev)
    e0.record()
    for _ in range(a.iters):
        launches(sink)
    e1.record()
    torch.cuda.synchronize()
    both_ms = e0.elapsed_time(e1) / a.iters
    hk, hn = ops.bleu_words(ids_d, tok_key, tail_key, tail_pow, sep_id, pad_id, tb["empty_key"])
    e0.record()
    for _ in range(a.iters):
        ops.bleu_counts(hk, hn, rk, rn, idx, counters=sink)
    e1.record()
    torch.cuda.synchronize()
    counts_ms = e0.elapsed_time(e1) / a.iters
    got = launches().cpu().tolist()

    host = []
    for _ in range(a.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = ids_d.cpu().tolist()
        want = C.string_counts([C.hyp_words(r, tokens) for r in rows], [t.split(" ") for t in refs])
        host.append(1e3 * (time.perf_counter() - t0))
    res = dict(config=f"n={a.n} tokens={a.tokens} V={V} reference words={a.tokens}", device=torch.cuda.get_device_name(0),
               words_and_counts_ms=both_ms, counts_ms=counts_ms, iters=a.iters, string_reference_ms=statistics.median(host),
               string_reference_runs=a.host_runs, counters=got, equal_to_string_reference=got == want,
               mean_hypothesis_words=got[8] / a.n, **RE.bleu_from_counters(got))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
