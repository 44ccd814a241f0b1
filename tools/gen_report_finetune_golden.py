"""Writes tests/golden/report_finetune_loss.npz: inputs and outputs of the upstream project's own LabelSmoothingLoss
(Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/loss.py), loaded by file path from a checkout of it.

    python tools/gen_report_finetune_golden.py --reference /path/to/MedViLL

Run by hand; no test imports this file or needs the checkout.  The golden holds numbers only: per case the logits f32 [B, P, V], the
labels int64 [B, P] (they include 0 and V - 1) and, for label_smoothing 0.1 and 1.0, the module's output [B, P] on
log_softmax(logits) -- the call of model.py:1047-1048 -- with the module converted by .double() and the log-probabilities handed over
in f64: the recorded numbers carry the module's own constants (the smoothing value torch.full rounded to f32 when the module was
built) and not the rounding of an f32 softmax and an f32 sum over V terms.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": (5, 4, 37), "b": (2, 3, 300)}
SMOOTHINGS = (0.1, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the upstream project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "report_finetune_loss.npz"))
    a = ap.parse_args()
    path = os.path.join(a.reference, "Downstream_task", "report_generation_and_vqa", "sc", "pytorch_pretrained_bert", "loss.py")
    spec = importlib.util.spec_from_file_location("_upstream_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, (B, P, V) in CASES.items():
        g = torch.Generator().manual_seed(1000 + V)
        z = torch.randn(B, P, V, generator=g) * 3.0
        labels = torch.randint(1, V - 1, (B, P), generator=g)
        labels[0, 0], labels[0, 1], labels[-1, -1] = 0, V - 1, 0
        out[f"{name}_logits"], out[f"{name}_labels"] = z.numpy(), labels.numpy()
        for ls in SMOOTHINGS:
            crit = mod.LabelSmoothingLoss(ls, V, ignore_index=0, reduction="none").double()
            with torch.no_grad():
                y = crit(torch.log_softmax(z.double(), dim=-1), labels)
            out[f"{name}_loss_{ls}"] = y.double().numpy()
    np.savez(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
