"""Write tests/golden/bertadam.npz FROM THE REFERENCE'S OWN BertAdam.

TEST INFRASTRUCTURE ONLY (CPU).  The reference module
Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/optimization.py is imported in place by path (MEDVILL_REFERENCE,
default as oracle/gen_golden.py) behind one shim -- `torch._six.container_abcs`, which current torch no longer has -- and stepped over a
FIXED recorded gradient sequence; nothing of it is copied.

    python tools/gen_bertadam_golden.py

Layout: six f32 tensors (SIZES) packed at 64-element aligned offsets, as the engine's flat buffer packs its parameters; two
parameter groups (DECAY marks the tensors of the weight-decay group).  `grads` [8, n] is the gradient sequence every case replays:
tensor 3's gradient norm is above max_grad_norm = 1 and tensor 5's below (both clip branches), tensor 1's gradient is all zero (it only
decays); in the `none_grad` case tensor 4 has NO gradient (`grad is None`: parameters, moments and step untouched -- and the
reference's get_lr() answers [0] as long as any Parameter has no state, so that case's `lr` is not a schedule value).
Per case c: `c/hyper` = [lr, warmup, t_total, b1, b2, e, weight_decay, max_grad_norm], `c/schedule`, `c/p` [steps, n] parameters after
every step, `c/lr` [steps] = get_lr()[0] after every step, `c/m`, `c/v` [n] the moments after the LAST step (every step's moments
enter the next step's parameters; storing them per step would put the file over its size budget).
`big/*`: a second layout, [4099, 65] elements, so that a tensor spans two of the kernels' 4,096-element chunks (a full chunk, then a
3-element last chunk) and the tensor behind it starts at chunk 2; constant lr, 2 steps, the large tensor's gradient norm ~ 10 (clipped).
Its inputs are multiples of 2^-15 / 2^-8 (exact in f32; they compress), its outputs are the parameters after each step.
`clip_spread`: max |p| difference over the `main` case between the reference as it is (f32 gradient norm) and the reference fed
gradients clipped beforehand by an f64 norm -- the reference's own sensitivity to the norm's summation order.
The reference's warmup_cosine calls torch.cos on a Python float after the warm-up, which raises under every torch that has the
function, so the `cosine` case stays inside the warm-up (t_total = 16); the product's post-warm-up branch is checked against the formula.
"""
from __future__ import annotations

import collections.abc
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF      # noqa: E402

SIZES = [2, 64, 65, 400, 130, 139]
DECAY = [False, True, False, True, True, False]
NONE_GRAD = 4
CASES = {
    "main": dict(warmup=0.25, t_total=8, schedule="warmup_linear", max_grad_norm=1.0, steps=8),
    "none_grad": dict(warmup=0.25, t_total=8, schedule="warmup_linear", max_grad_norm=1.0, steps=3, none=True),
    "const_lr": dict(warmup=-1, t_total=-1, schedule="warmup_linear", max_grad_norm=1.0, steps=3),
    "noclip": dict(warmup=0.25, t_total=8, schedule="warmup_linear", max_grad_norm=-1, steps=3),
    "constant": dict(warmup=0.25, t_total=8, schedule="warmup_constant", max_grad_norm=1.0, steps=3),
    "cosine": dict(warmup=0.25, t_total=16, schedule="warmup_cosine", max_grad_norm=1.0, steps=3),
}
LR, WD = 1e-2, 0.01
BIG_SIZES, BIG_DECAY = [4096 + 3, 65], [True, False]
BIG = dict(warmup=-1, t_total=-1, schedule="warmup_linear", max_grad_norm=1.0, steps=2)


def reference_module():
    six = types.ModuleType("torch._six")
    six.container_abcs = collections.abc
    sys.modules["torch._six"] = six
    path = os.path.join(REF, "Downstream_task", "report_generation_and_vqa", "sc", "pytorch_pretrained_bert", "optimization.py")
    spec = importlib.util.spec_from_file_location("_ref_optimization", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def offsets(sizes=None):
    offs, off = [], 0
    for n in (SIZES if sizes is None else sizes):
        offs.append(off)
        off = (off + n + 63) // 64 * 64
    return offs, off


def pack(ts, offs, n):
    out = np.zeros(n, dtype=np.float32)
    for t, o in zip(ts, offs):
        out[o:o + t.numel()] = t.detach().numpy().reshape(-1)
    return out


def run(mod, p0, grads, offs, n, cfg, preclip64=False, SIZES=SIZES, DECAY=DECAY):
    params = [torch.nn.Parameter(torch.from_numpy(p0[o:o + s].copy())) for o, s in zip(offs, SIZES)]
    groups = [{"params": [p for p, d in zip(params, DECAY) if d], "weight_decay": WD},
              {"params": [p for p, d in zip(params, DECAY) if not d], "weight_decay": 0.0}]
    mgn = cfg["max_grad_norm"]
    opt = mod.BertAdam(groups, lr=LR, warmup=cfg["warmup"], t_total=cfg["t_total"], schedule=cfg["schedule"],
                       max_grad_norm=-1 if preclip64 else mgn)
    ps, lrs = [], []
    for s in range(cfg["steps"]):
        for i, (p, o, sz) in enumerate(zip(params, offs, SIZES)):
            if i == NONE_GRAD and cfg.get("none"):
                p.grad = None
                continue
            g = torch.from_numpy(grads[s, o:o + sz].copy())
            if preclip64 and mgn > 0:
                g = (g.double() * min(1.0, mgn / (float(g.double().pow(2).sum().sqrt()) + 1e-6))).float()
            p.grad = g
        opt.step()
        ps.append(pack(params, offs, n))
        lrs.append(float(opt.get_lr()[0]))
    zeros = lambda p: torch.zeros_like(p)
    m = pack([opt.state[p].get("next_m", zeros(p)) for p in params], offs, n)
    v = pack([opt.state[p].get("next_v", zeros(p)) for p in params], offs, n)
    return np.stack(ps), np.asarray(lrs, dtype=np.float64), m, v


def main():
    mod = reference_module()
    offs, n = offsets()
    rng = np.random.RandomState(20240607)
    p0 = np.zeros(n, dtype=np.float32)
    grads = np.zeros((8, n), dtype=np.float32)
    scale = [1.0, 0.0, 0.05, 0.14, 0.03, 0.02]          # tensor 3: norm ~ 2.8 (clipped); tensor 5: ~ 0.24 (not); tensor 1: zero gradient
    for o, s, sc in zip(offs, SIZES, scale):
        p0[o:o + s] = rng.standard_normal(s).astype(np.float32) * 0.5
        grads[:, o:o + s] = rng.standard_normal((8, s)).astype(np.float32) * sc
    out = dict(sizes=np.asarray(SIZES, dtype=np.int64), offsets=np.asarray(offs, dtype=np.int64), decay=np.asarray(DECAY),
               none_grad=np.asarray(NONE_GRAD), p0=p0, grads=grads, cases=np.asarray(list(CASES)))
    for name, cfg in CASES.items():
        ps, lrs, m, v = run(mod, p0, grads, offs, n, cfg)
        out[f"{name}/hyper"] = np.asarray([LR, cfg["warmup"], cfg["t_total"], 0.9, 0.999, 1e-6, WD, cfg["max_grad_norm"]], dtype=np.float64)
        out[f"{name}/schedule"] = np.asarray(cfg["schedule"])
        out[f"{name}/p"], out[f"{name}/lr"], out[f"{name}/m"], out[f"{name}/v"] = ps, lrs, m, v
    ps64 = run(mod, p0, grads, offs, n, CASES["main"], preclip64=True)[0]
    out["clip_spread"] = np.asarray(float(np.abs(ps64 - out["main/p"]).max()))
    # `big`: a layout of its own whose first tensor spans more than one kernel chunk (4,096 elements) and ends on a 3-element tail
    boffs, bn = offsets(BIG_SIZES)
    bp0, bg = np.zeros(bn, dtype=np.float32), np.zeros((BIG["steps"], bn), dtype=np.float32)
    for o, s, gq in zip(boffs, BIG_SIZES, (40.0, 1.5)):
        bp0[o:o + s] = np.round(rng.standard_normal(s) * 8192).clip(-32767, 32767).astype(np.float32) / 32768.0
        bg[:, o:o + s] = np.round(rng.standard_normal((BIG["steps"], s)) * gq).clip(-127, 127).astype(np.float32) / 256.0
    ps, lrs, _, _ = run(mod, bp0, bg, boffs, bn, BIG, SIZES=BIG_SIZES, DECAY=BIG_DECAY)
    out.update({"big/sizes": np.asarray(BIG_SIZES, dtype=np.int64), "big/offsets": np.asarray(boffs, dtype=np.int64),
                "big/decay": np.asarray(BIG_DECAY), "big/p0": bp0, "big/grads": bg, "big/p": ps, "big/lr": lrs,
                "big/schedule": np.asarray(BIG["schedule"]),
                "big/hyper": np.asarray([LR, BIG["warmup"], BIG["t_total"], 0.9, 0.999, 1e-6, WD, BIG["max_grad_norm"]], dtype=np.float64)})
    path = os.path.join(ROOT, "tests", "golden", "bertadam.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; clip_spread", float(out["clip_spread"]))
    for name in CASES:
        print(name, "lr", out[f"{name}/lr"])


if __name__ == "__main__":
    main()
