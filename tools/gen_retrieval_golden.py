"""Writes tests/golden/retrieval_metrics.npz: inputs and recorded outputs of the upstream project's own compute_ranks,
compute_recall_precision and compute_mrr (Downstream_task/Retrieval/full_dset_retrieval.py), taken from a checkout of it.

    python tools/gen_retrieval_golden.py --reference /path/to/MedViLL

Run by hand; no test imports this file or needs the checkout.  The upstream module cannot be imported as a whole without its logging,
string-matching and tokenizer dependencies, so the three function definitions are cut out of its syntax tree at run time and compiled
on their own, with numpy as their only global.  The golden holds numbers only: per case the scores f32 [G*C] (distinct within a group),
the labels (every group holds an aligned candidate), the candidate ids, the group size, and what the functions returned -- ranks,
Aligned_lst, recall@{1,5,10} and precision@{1,5,10} as the upstream dictionaries hold them (rounded to 3 decimals there), and the MRR.
"""
import argparse
import ast
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTED = ("compute_ranks", "compute_recall_precision", "compute_mrr")
CASES = {"a": (40, 10, "one"), "b": (12, 100, "several"), "c": (25, 7, "mixed")}        # G, C, aligned candidates per group


def load_functions(path):
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED), [d.name for d in defs]
    ns = {"np": np}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in WANTED]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the upstream project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "retrieval_metrics.npz"))
    a = ap.parse_args()
    ranks_fn, rp_fn, mrr_fn = load_functions(os.path.join(a.reference, "Downstream_task", "Retrieval", "full_dset_retrieval.py"))
    out = {}
    for name, (G, C, kind) in CASES.items():
        rng = np.random.default_rng(100 + G + C)
        sims = np.stack([rng.permutation(C) for _ in range(G)]).astype(np.float32) / np.float32(C) + np.float32(0.001)   # distinct per group
        labels = np.zeros((G, C), dtype=np.int64)
        for g in range(G):
            k = 1 if kind == "one" else (int(rng.integers(2, 9)) if kind == "several" else int(rng.integers(1, C + 1)))
            labels[g, rng.choice(C, size=k, replace=False)] = 1
        ids = rng.permutation(G * C).astype(np.int64)
        args = SimpleNamespace(eval_len_size=C, i2t=True, t2i=False)
        res, lab, idl = [np.float32(v) for v in sims.reshape(-1)], labels.reshape(-1).tolist(), ids.tolist()
        with contextlib.redirect_stdout(io.StringIO()):
            i2t, _, aligned = ranks_fn(args, res, lab, idl)
            rp = rp_fn(args, res, lab, idl)
            mrr = mrr_fn(i2t)
        out[f"{name}_sims"], out[f"{name}_labels"], out[f"{name}_ids"], out[f"{name}_C"] = sims.reshape(-1), labels.reshape(-1), ids, np.int64(C)
        out[f"{name}_ranks"] = np.asarray(i2t, dtype=np.int64)
        out[f"{name}_aligned"] = np.asarray(aligned, dtype=np.int64)
        out[f"{name}_recall"] = np.asarray([rp["i2t_recall"][k] for k in ("R@1", "R@5", "R@10")], dtype=np.float64)
        out[f"{name}_precision"] = np.asarray([rp["i2t_precision"][k] for k in ("R@1", "R@5", "R@10")], dtype=np.float64)
        out[f"{name}_mrr"] = np.float64(mrr)
    np.savez(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
