"""Sweep of the batch-assembly and row-plan kernels (csrc/mv_batch.hip: mv_mlm_draws, mv_mlm_corrupt with its label-index pass,
mv_pack_plan, mv_tail_perm) over the cases of tests/batch_cases.py, against the plain references there.  batch_cases.py holds the
judgement of every family; tests/test_batch_cases_cpu.py proves which branch every case takes and that the judgement catches each
planted defect.  Every case runs: nothing here may drop one.

The library is called through the C ABI with buffers of the test's own (the hip_ops wrappers allocate their outputs, which cannot be
guarded): every output sits between guard elements in a buffer pre-filled with a sentinel -- an integer no result can be, NaN for u.
After the call the elements the contract writes hold the reference's values, exactly, and everything else still holds the sentinel:
the guards, rowmap / perm / newpos from cu[B] on, the index buffers from n_labels on, and desc and the index buffers when NULL was
passed in their place.  The last test runs the wrappers on the chain cases against the direct calls.  The assertion messages carry
the cfg dict, which reproduces the case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import data                  # noqa: E402
from medvill_amd import hip_ops as ops        # noqa: E402

import batch_cases as C                       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH_DT = {C.I32: torch.int32, C.I64: torch.int64, C.F32: torch.float32}


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Bufs:
    """the device side of batch_cases.new_buffers: name -> sentinel-filled flat tensor; t(name) is the part the kernel is handed"""

    def __init__(self, specs):
        self.specs = dict(specs)
        self.flat = {k: torch.full((n + 2 * C.GUARD,), float("nan") if dt is C.F32 else C.SENTINEL, dtype=TORCH_DT[dt], device=DEV)
                     for k, (dt, n) in specs.items()}

    def add(self, specs):
        more = Bufs(specs)
        self.specs.update(more.specs)
        self.flat.update(more.flat)

    def t(self, name):
        return self.flat[name][C.GUARD:C.GUARD + self.specs[name][1]]

    def p(self, name, given=True):
        return self.t(name).data_ptr() if given else None

    def host(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.flat.items()}


def call(name, *args):
    ops.L.check(getattr(ops._lib(), name)(*args, ops.L.stream_ptr()), name)


def run_draws(bufs, names, key, B, S, vocab):
    call("mv_mlm_draws", key, B, S, vocab, bufs.p(names[0]), bufs.p(names[1]))


def run_corrupt(bufs, B, N, S, ids, lengths, u, rnd, family, desc=True, index=True):
    call("mv_mlm_corrupt", ids.data_ptr(), lengths.data_ptr(), u.data_ptr(), rnd.data_ptr(), None if family is None else family.data_ptr(), B, N, S,
         bufs.p("input_txt"), bufs.p("segment"), bufs.p("txt_labels"), bufs.p("n_ids"), bufs.p("desc", desc), bufs.p("counts"),
         bufs.p("label_rows", index), bufs.p("label_ids", index), bufs.p("n_labels", index))


def run_pack(bufs, B, L, desc):
    call("mv_pack_plan", desc.data_ptr(), B, L, bufs.p("cu"), bufs.p("rowmap"), bufs.p("inv"))


def run_tail(bufs, B, L, cu, sel):
    call("mv_tail_perm", cu.data_ptr(), B, L, sel.data_ptr(), int(sel.numel()), bufs.p("perm"), bufs.p("newpos"), bufs.p("qlim"), bufs.p("sel_new"))


def settle(cfg, verdict, inputs_intact=True):
    ok, what = verdict
    assert ok and inputs_intact, (what, cfg, C.FAMILIES[cfg["fam"]][1](cfg))


@pytest.mark.parametrize("cfg", C.draws_cases(), ids=C.case_id)
def test_mlm_draws_cases(cfg):
    inp = C.draws_inputs(cfg)
    bufs = Bufs(C.draws_buffers(cfg))
    run_draws(bufs, ("u", "rnd"), inp["key"], cfg["B"], cfg["S"], inp["vocab"])
    if C.draws_shape2(cfg):
        run_draws(bufs, ("u2", "rnd2"), inp["key"], *C.draws_shape2(cfg), inp["vocab"])
    settle(cfg, C.draws_judge(cfg, inp, C.draws_reference(cfg, inp), bufs.host()))


@pytest.mark.parametrize("cfg", C.corrupt_cases(), ids=C.case_id)
def test_mlm_corrupt_cases(cfg):
    inp = C.corrupt_inputs(cfg)
    bufs = Bufs(C.corrupt_buffers(cfg))
    d = {k: dev(inp[k]) for k in ("ids", "lengths", "u", "rnd", "family")}
    run_corrupt(bufs, cfg["B"], cfg["N"], cfg["S"], d["ids"], d["lengths"], d["u"], d["rnd"], d["family"], cfg["desc"] == "given", cfg["index"] == "given")
    out = bufs.host()
    intact = all(d[k] is None or np.array_equal(d[k].cpu().numpy().view(np.int32), np.ascontiguousarray(inp[k]).view(np.int32)) for k in d)
    settle(cfg, C.corrupt_judge(cfg, inp, C.corrupt_reference(cfg, inp), out), intact)


@pytest.mark.parametrize("cfg", C.pack_cases(), ids=C.case_id)
def test_pack_plan_cases(cfg):
    inp = C.pack_inputs(cfg)
    bufs = Bufs(C.pack_buffers(cfg))
    desc = dev(inp["desc"])
    run_pack(bufs, cfg["B"], cfg["L"], desc)
    out = bufs.host()
    settle(cfg, C.pack_judge(cfg, inp, C.pack_reference(cfg, inp), out), np.array_equal(desc.cpu().numpy(), inp["desc"]))


@pytest.mark.parametrize("cfg", C.tail_cases(), ids=C.case_id)
def test_tail_perm_cases(cfg):
    inp = C.tail_inputs(cfg)
    bufs = Bufs(C.tail_buffers(cfg, inp))
    cu, sel = dev(inp["cu"]), dev(inp["sel"])
    run_tail(bufs, inp["B"], cfg["L"], cu, sel)
    out = bufs.host()
    intact = np.array_equal(cu.cpu().numpy(), inp["cu"]) and np.array_equal(sel.cpu().numpy(), inp["sel"])
    settle(cfg, C.tail_judge(cfg, inp, C.tail_reference(cfg, inp), out), intact)


def run_chain(cfg, inp):
    """the engine's composition through the C ABI: every stage reads the device buffers of the one before it; only the two sizes
    (n_labels, cu[B]) come to the host"""
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    L = S + N + 3
    specs = C._chain_sizes(cfg, 0, 0)
    bufs = Bufs({k: v for k, v in specs.items() if k not in ("perm", "newpos", "qlim", "sel_new")})
    ids, lengths, family = dev(inp["ids"]), dev(inp["lengths"]), dev(inp["family"])
    run_draws(bufs, ("u", "rnd"), inp["key"], B, S, inp["vocab"])
    run_corrupt(bufs, B, N, S, ids, lengths, bufs.t("u"), bufs.t("rnd"), family)
    run_pack(bufs, B, L, bufs.t("desc"))
    n, M = int(bufs.t("n_labels").item()), int(bufs.t("cu")[B].item())
    assert 0 <= n <= B * S and 0 <= M <= B * L, (n, M, cfg)
    rows = torch.tensor(C.chain_tail_rows(cfg, bufs.t("label_rows").cpu().numpy(), n), dtype=torch.int64, device=DEV)
    sel = torch.cat([bufs.t("inv").index_select(0, rows), bufs.t("cu")[:B]]).contiguous()
    bufs.add({k: v for k, v in C._chain_sizes(cfg, n, M).items() if k in ("perm", "newpos", "qlim", "sel_new")})
    run_tail(bufs, B, L, bufs.t("cu"), sel)
    out = bufs.host()
    out["sel"] = sel.cpu().numpy()
    return bufs, out


@pytest.mark.parametrize("cfg", C.chain_cases(), ids=C.case_id)
def test_chain_cases(cfg):
    inp = C.chain_inputs(cfg)
    _, out = run_chain(cfg, inp)
    settle(cfg, C.chain_judge(cfg, inp, C.chain_reference(cfg, inp), out))


@pytest.mark.parametrize("cfg", C.chain_cases(), ids=C.case_id)
def test_the_wrappers_equal_the_direct_calls_on_the_chain(cfg):
    """ops.mlm_draws / mlm_corrupt / pack_plan / tail_perm and data.assemble_batch: their shape and dtype handling, and what they return"""
    inp = C.chain_inputs(cfg)
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    L = S + N + 3
    bufs, out = run_chain(cfg, inp)
    n, M = int(bufs.t("n_labels").item()), int(bufs.t("cu")[B].item())
    ids, lengths, family = dev(inp["ids"]), dev(inp["lengths"]), dev(inp["family"])
    u, rnd = ops.mlm_draws(inp["key"], B, S, inp["vocab"], DEV)
    assert u.shape == rnd.shape == (B, S) and torch.equal(u.view(-1), bufs.t("u")) and torch.equal(rnd.view(-1), bufs.t("rnd")), cfg
    c = ops.mlm_corrupt(ids, lengths, u, rnd, N, family=family)
    for k, shape in (("input_txt", (B, S + 1)), ("segment", (B, S + 1)), ("txt_labels", (B, L)), ("n_ids", (B,)), ("desc", (B, 3)), ("counts", (B,)),
                     ("n_labels", (1,))):
        assert tuple(c[k].shape) == shape and c[k].dtype == bufs.t(k).dtype and torch.equal(c[k].reshape(-1), bufs.t(k)), (k, cfg)
    for k in ("label_rows", "label_ids"):
        assert c[k].numel() >= B * S and torch.equal(c[k][:n], bufs.t(k)[:n]), (k, cfg)
    assert set(ops.mlm_corrupt(ids, lengths, u, rnd, N, want_index=False)) == {"input_txt", "segment", "txt_labels", "n_ids", "desc", "counts"}
    a = data.assemble_batch(ids, lengths.to(torch.int64), N, inp["vocab"], key=inp["key"], family=inp["fams"])
    for k in ("input_txt", "segment", "txt_labels"):
        assert torch.equal(a[k].reshape(-1), bufs.t(k)), (k, cfg)
    assert a["n_ids"].dtype == torch.int64 and torch.equal(a["n_ids"].to(torch.int32), bufs.t("n_ids")), cfg
    assert a["label_rows"].numel() == n and torch.equal(a["label_rows"], bufs.t("label_rows")[:n]) and torch.equal(a["label_ids"], bufs.t("label_ids")[:n])
    assert a["attn_desc"].L == L and torch.equal(a["attn_desc"].desc.reshape(-1), bufs.t("desc")), cfg
    cu, rowmap, inv = ops.pack_plan(c["desc"], B, L)
    assert torch.equal(cu, bufs.t("cu")) and torch.equal(rowmap[:M], bufs.t("rowmap")[:M]) and torch.equal(inv, bufs.t("inv")), cfg
    sel = torch.from_numpy(out["sel"]).to(DEV)
    perm, newpos, qlim, sel_new = ops.tail_perm(cu, B, L, sel, M)
    assert perm.numel() == newpos.numel() == M and torch.equal(perm, bufs.t("perm")[:M]) and torch.equal(newpos, bufs.t("newpos")[:M]), cfg
    assert torch.equal(qlim, bufs.t("qlim")) and torch.equal(sel_new, bufs.t("sel_new")), cfg
    with pytest.raises(TypeError):
        ops.tail_perm(cu, B, L, sel.to(torch.int64), M)
    with pytest.raises(TypeError):
        ops.pack_plan(c["desc"].to(torch.int64), B, L)
    with pytest.raises(ValueError):
        ops.mlm_corrupt(ids, lengths[:-1], u, rnd, N)
