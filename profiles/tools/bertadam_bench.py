"""Time mv_tensor_sqnorms + mv_bertadam_step against mv_adamw_step on the same BERT-base flat buffers, and both against their byte
models (AdamW reads p, g, m, v and writes p, m, v and the two 16-bit copies: 32 bytes per element; BertAdam reads g once more: 36).
The rates are byte-model bytes over time: part of the second read of g comes from the last-level cache, so they are not HBM figures.

    python profiles/tools/bertadam_bench.py [--reps 20] [--out profiles/bertadam_bench.json]

Device events around each call after warm-up calls; median, minimum and maximum over the repetitions are reported."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from medvill_amd import hip_ops as ops                      # noqa: E402
from medvill_amd.engine import ModelConfig, param_layout   # noqa: E402
from medvill_amd.optim import build_tables                 # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lay, n = param_layout(ModelConfig())
    entries = [(off, math.prod(shape), not name.endswith("bias") and "LayerNorm" not in name, True) for name, (off, shape) in lay.items()]
    n_el = sum(e[1] for e in entries)
    t, c = build_tables(entries)
    t, c = t.to(dev), c.to(dev)
    p = torch.randn(n, device=dev) * 0.02
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sh, shf = torch.zeros(n, device=dev, dtype=torch.bfloat16), torch.zeros(n, device=dev, dtype=torch.float16)
    part, sq = torch.zeros(c.numel(), device=dev), torch.zeros(t.shape[0], device=dev)
    step = [0]

    def adamw():
        step[0] += 1
        ops.adamw_step(p, g, m, v, sh, n, 1e-5, 0.9, 0.999, 1e-6, 0.01, step[0], shadow_f16=shf)

    def norms():
        ops.tensor_sqnorms(g, t, c, part, sq)

    def bertadam():
        ops.tensor_sqnorms(g, t, c, part, sq)
        ops.bertadam_step(p, g, m, v, t, c, sq, lr=1e-5, step=5, warmup=0.1, t_total=1000, shadow=sh, shadow_f16=shf)

    res = dict(arch=torch.cuda.get_device_properties(0).gcnArchName, elements=n_el, flat_elements=n, tensors=len(entries), chunks=int(c.numel()), reps=a.reps,
               note="single session; device events around each call; gb_per_s is bytes of the byte model over time, not an HBM figure: "
                    "the re-read of g and the 16-bit copies can be served by the 256 MB last-level cache")
    for name, fn, nbytes in (("adamw", adamw, 32 * n_el), ("sqnorms", norms, 4 * n_el), ("bertadam", bertadam, 36 * n_el)):
        us = timed(fn, a.reps)
        med = statistics.median(us)
        res[name] = dict(median_us=med, min_us=min(us), max_us=max(us), bytes=nbytes, gb_per_s=nbytes / med / 1e3)
    res["bertadam_over_adamw"] = res["bertadam"]["median_us"] / res["adamw"]["median_us"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
