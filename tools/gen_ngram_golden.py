"""Write tests/golden/ngram_beam.npz FROM THE REFERENCE'S OWN beam search with n-gram blocking.

TEST INFRASTRUCTURE ONLY (CPU), run by hand:

    python tools/gen_ngram_golden.py

The reference's Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py cannot be imported here (it needs
torchvision and einops), so the source of BertForSeq2SeqDecoder.beam_search -- the whole method, its nested candidate function
included -- is cut out of the reference checkout (MEDVILL_REFERENCE, default as oracle/gen_golden.py) with `ast` AT RUN TIME,
compiled, and bound to a stand-in object whose `bert` / `cls` return recorded score tables instead of running a model.  Two
in-process shims make it run on the CPU: Tensor.cuda() returns the tensor, torch.cuda.LongTensor is torch.LongTensor.  Nothing of
the reference's text is held here or written out: the fixture holds numbers only.

Per case c: `c/tables` f32 [steps, B*K, V] (the scores `cls` answers at step t for beam row r; at step 0, when the reference still
runs one row per sample, sample b reads row b*K), the parameters (`B`, `K`, `V`, `n`, `steps`, `min_len`, `length_penalty`,
`eos_id`, `ignore` int64 [m]) and what the method returned: `pred_seq` [B, T], `scores` [B, T, K], `wids`, `ptrs` (T = 1 + steps, the
reference pads to its output length).  The method never stops early: every case runs all its steps.

The tool asserts that every case's traces differ from the same run without blocking, and that no chosen candidate lies within 1e-3
of the next one (neither top-k has a tie to break): for that it replays the run with the rule of tests/ngram_cases.py.
"""
from __future__ import annotations

import ast
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import REF      # noqa: E402
import ngram_cases as NC               # noqa: E402

MODEL_PY = os.path.join(REF, "Downstream_task", "report_generation_and_vqa", "sc", "pytorch_pretrained_bert", "model.py")
OUT = os.path.join(ROOT, "tests", "golden", "ngram_beam.npz")
EOS = 5
MIN_GAP = 1e-3
FLOOR = -30000.0                       # a score no penalised column falls below: lets the held-back EOS column (-10000) be chosen

# name: B, K, V, n, steps, min_len, length penalty, ignore ids, (step, amount) added to the EOS score from that step on, noise seed
CASES = {
    "k4_n2": dict(B=2, K=4, V=24, n=2, steps=10, min_len=0, lp=0.0, ignore=[], eos=(6, 3.0), seed=0),
    "k4_n3_ignore": dict(B=2, K=4, V=24, n=3, steps=12, min_len=0, lp=0.0, ignore=[7, 11], eos=(8, 3.0), seed=2),
    "k4_n2_ignore": dict(B=1, K=4, V=32, n=2, steps=10, min_len=0, lp=0.0, ignore=[3, 9, 20], eos=(20, 0.0), seed=0),
    "k3_n2_min_len_lp": dict(B=2, K=3, V=32, n=2, steps=10, min_len=3, lp=0.5, ignore=[], eos=(0, 4.0), seed=1),
    "k3_n4": dict(B=1, K=3, V=24, n=4, steps=14, min_len=0, lp=0.0, ignore=[], eos=(20, 0.0), seed=0),
    "k3_n3_lp": dict(B=2, K=3, V=40, n=3, steps=12, min_len=2, lp=-0.3, ignore=[4], eos=(5, 2.5), seed=1),
    "k1_n2": dict(B=3, K=1, V=24, n=2, steps=10, min_len=0, lp=0.0, ignore=[], eos=(4, 2.0), seed=0),
    "k1_n3_ignore": dict(B=2, K=1, V=28, n=3, steps=12, min_len=0, lp=0.0, ignore=[2], eos=(20, 0.0), seed=0),
    "k1_n4": dict(B=1, K=1, V=24, n=4, steps=14, min_len=0, lp=0.0, ignore=[], eos=(20, 0.0), seed=0),
    # EOS both banned and held back by min_len: the beam a, EOS, a at step 3 < min_len (see crafted_tables); it extends after EOS too
    "k1_n2_eos_banned_in_min_len": dict(B=1, K=1, V=24, n=2, steps=7, min_len=4, lp=0.0, ignore=[], eos=(20, 0.0), seed=0, crafted=True),
}


def make_tables(c):
    """scores with a few favourite words per row (so that an unblocked search repeats itself), f32 [steps, B*K, V]"""
    g = torch.Generator().manual_seed(1000 + c["seed"])
    B, K, V, steps = c["B"], c["K"], c["V"], c["steps"]
    fav = torch.randn((B, 1, V), generator=g).repeat(1, K, 1).reshape(1, B * K, V) * 2.5
    x = fav + torch.randn((steps, B * K, V), generator=g) * (1.0 if c["n"] < 4 else 0.6)
    t0, amount = c["eos"]
    x[t0:, :, EOS] += amount
    if c.get("crafted"):
        a = 9
        noise = x * 0.05
        x = torch.zeros_like(x)
        x[0, :, a] = 8.0                                   # step 0: a
        x[1] = FLOOR                                       # step 1: nothing but EOS, which min_len holds at -10000: EOS is chosen
        x[1, :, EOS] = 0.0
        x[2, :, a] = 8.0                                   # step 2: a again -> the history a, EOS, a bans EOS at step 3
        x[3] = FLOOR
        x[3, :, EOS] = 0.0                                 # step 3: EOS banned and held back: -10000 exactly, and chosen
        x[4:, :, a] = 8.0                                  # from step 4 on: a is banned after EOS, a (n = 2)
        x = x + noise
    return x.float().contiguous()


def reference_beam_search():
    """the method, compiled from the reference checkout's text"""
    tree = ast.parse(open(MODEL_PY).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BertForSeq2SeqDecoder")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "beam_search")
    mod = ast.Module(body=[fn], type_ignores=[])
    ns = {"torch": torch, "np": np, "math": math, "F": torch.nn.functional, "nn": torch.nn}
    exec(compile(mod, MODEL_PY, "exec"), ns)
    return ns["beam_search"]


class StandIn:
    """what beam_search reads of its model: the search parameters, and `bert` / `cls` answering from the tables"""

    def __init__(self, c, tables, blocking):
        self.search_beam_size, self.length_penalty, self.eos_id, self.min_len = c["K"], c["lp"], EOS, c["min_len"]
        self.forbid_duplicate_ngrams, self.forbid_ignore_set, self.ngram_size = blocking, set(c["ignore"]) or None, c["n"]
        self.mask_word_id, self.len_vis_input = 1, None
        self.tables, self.K, self.step = tables, c["K"], 0

    def bert(self, vis_feats, x_input_ids, *a, **k):
        rows, cols = x_input_ids.shape
        h = torch.zeros((rows, cols, 1))
        return h, [h], None

    def cls(self, last_hidden, *a, **k):
        t = self.tables[self.step]
        self.step += 1
        if last_hidden.shape[0] != t.shape[0]:             # step 0: one row per sample
            t = t[::self.K]
        return t.clone().unsqueeze(1), None


def run_reference(fn, c, tables, blocking):
    B, steps = c["B"], c["steps"]
    T = 1 + steps
    obj = StandIn(c, tables, blocking)
    ids = torch.zeros((B, 1), dtype=torch.long)
    tt = torch.zeros((B, T), dtype=torch.long)
    pos = torch.arange(T).unsqueeze(0).repeat(B, 1)
    am = torch.ones((B, T, T), dtype=torch.long)
    tr = types.MethodType(fn, obj)(None, ids, tt, pos, am, None, "cpu")
    assert obj.step == steps
    return {k: v.numpy() for k, v in tr.items()}


def check_no_ties(c, tables, tr):
    """replay with the restated rule along the reference's own choices: every top-k decision has a margin above MIN_GAP"""
    B, K, n = c["B"], c["K"], c["n"]
    seqs = [[] for _ in range(B * K)]
    scores = eos_mask = None
    for t in range(c["steps"]):
        lp = torch.log_softmax(tables[t], dim=-1)
        for r, s in enumerate(seqs):
            for w in NC.banned_words(s, n, c["ignore"]):
                lp[r, w] += -10000.0
        if t < c["min_len"]:
            lp[:, EOS] = -10000.0
        kk, _ = torch.topk(lp, k=K + 1)
        rows = range(0, B * K, K) if t == 0 else range(B * K)
        for r in rows:
            assert float((kk[r, :-1] - kk[r, 1:]).min()) > MIN_GAP, (t, r)
        if t > 0:
            cand = (kk[:, :K] + (eos_mask * -10000.0 + scores).reshape(-1, 1)).reshape(B, K * K)
            top = torch.sort(cand, dim=1, descending=True).values[:, :min(K * K, K + 1)]
            assert K == 1 or float((top[:, :-1] - top[:, 1:]).min()) > MIN_GAP, t
        w, p = torch.from_numpy(tr["wids"][:, t]), torch.from_numpy(tr["ptrs"][:, t])
        par = (torch.arange(B).unsqueeze(1) * K + p).reshape(-1)
        seqs = [[int(x)] for x in w.reshape(-1)] if t == 0 else NC.step_histories(seqs, par, w.reshape(-1))
        scores, eos_mask = torch.from_numpy(tr["scores"][:, t]), (w == EOS).float()


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self         # in-process shims: the method moves its ban mask and back pointers to a GPU
    torch.cuda.LongTensor = torch.LongTensor
    fn = reference_beam_search()
    out = {}
    for name, c in CASES.items():
        tables = make_tables(c)
        tr = run_reference(fn, c, tables, True)
        off = run_reference(fn, c, tables, False)
        assert not np.array_equal(tr["wids"], off["wids"]), f"{name}: blocking changes nothing"
        check_no_ties(c, tables, tr)
        out[f"{name}/tables"] = tables.numpy()
        for k, v in (("B", c["B"]), ("K", c["K"]), ("V", c["V"]), ("n", c["n"]), ("steps", c["steps"]), ("min_len", c["min_len"]), ("eos_id", EOS)):
            out[f"{name}/{k}"] = np.int64(v)
        out[f"{name}/length_penalty"] = np.float64(c["lp"])
        out[f"{name}/ignore"] = np.asarray(c["ignore"], dtype=np.int64)
        out[f"{name}/pred_seq"] = tr["pred_seq"].astype(np.int64)
        out[f"{name}/scores"] = tr["scores"].astype(np.float32)
        out[f"{name}/wids"] = tr["wids"].astype(np.int64)
        out[f"{name}/ptrs"] = tr["ptrs"].astype(np.int64)
        print(f"{name}: {tables.numel() * 4} bytes of tables; first sample: {tr['pred_seq'][0].tolist()}")
    if os.path.exists(OUT):                                # (the zip container carries a time stamp: compare the arrays, not the file)
        old = np.load(OUT)
        same = set(old.files) == set(out) and all(np.asarray(out[k]).tobytes() == old[k].tobytes() and np.asarray(out[k]).dtype == old[k].dtype for k in out)
        print("arrays bit-identical to the committed fixture" if same else "ARRAYS DIFFER from the committed fixture")
    with open(OUT, "wb") as f:
        np.savez_compressed(f, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
