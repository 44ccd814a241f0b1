"""Sweep of the fine-tuning loss and optimizer kernels (csrc/mv_lmloss.hip: mv_lm_loss_fwd / _select / _bwd; csrc/mv_vqa.hip:
mv_bce_fwd_bwd, mv_rows_mul; csrc/mv_optim.hip: mv_tensor_sqnorms, mv_bertadam_step, mv_bce_multilabel) over the cases of
tests/headops_cases.py, against float64 references with one bound per output element.  headops_cases.py derives the bounds and holds
the judgement of every family; tests/test_headops_cases_cpu.py shows that the bounds let an honest f32 computation through and catch
each planted defect, and proves which branch every case takes.  Every case runs: nothing here may drop one.

Per case: every output that has a leading dimension sits inside a NaN-filled buffer with guard elements in front and behind (moved
by the case's base offset), pad columns of the inputs hold NaN or 1e30, and whatever lies outside the logical extent must come back
with its bits.  The inputs are made on the host from the cfg alone; the outputs are judged on the host.  The last test prints the
worst error / bound of every family.  The assertion messages carry the cfg dict, which reproduces the case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402
from medvill_amd import optim as mv_optim     # noqa: E402

import headops_cases as C                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}


def dev(x):
    """host numpy / torch -> device tensor (None stays None)"""
    if x is None:
        return None
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(DEV)


class Buf:
    """rows x cols of `dtype` inside a NaN-filled device buffer: C.GUARD + off elements in front, C.GUARD behind"""

    def __init__(self, rows, cols, dtype, off=0, init=None):
        self.lo = C.GUARD + off
        self.hi = self.lo + rows * cols
        self.flat = torch.full((self.hi + C.GUARD,), C.NAN, dtype=dtype, device=DEV)
        self.t = self.flat[self.lo:self.hi].view(rows, cols)
        if init is not None:
            self.t.copy_(dev(init))
        self.before = self.flat.clone()

    def guards_ok(self):
        return torch.equal(C.bits(self.flat[:self.lo]), C.bits(self.before[:self.lo])) and \
            torch.equal(C.bits(self.flat[self.hi:]), C.bits(self.before[self.hi:]))

    def unchanged(self):
        return torch.equal(C.bits(self.flat), C.bits(self.before))


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


def settle(cfg, verdict, extra=True):
    ok, worst, what = verdict
    key = cfg["fam"] + "/" + str(cfg.get("ddt", cfg.get("dt", C.F32)))                       # by output encoding: a 16-bit store reaches its half ulp
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"{C.case_id(cfg)}: error / bound {worst:.4f}")
    assert ok and extra, (what, "error / bound = %.3g" % worst, cfg, C.FAMILIES[cfg["fam"]][1](cfg))


@pytest.mark.parametrize("cfg", C.rmul_cases(), ids=C.case_id)
def test_rows_mul_cases(cfg):
    inp = C.rmul_inputs(cfg)
    H, R, ld = cfg["H"], cfg["R"], inp["ld"]
    a = Buf(inp["a"].shape[0], ld, C.DT[cfg["dt"]], init=inp["a"])
    b = a if cfg["same"] else Buf(inp["b"].shape[0], ld, C.DT[cfg["dt"]], init=inp["b"])
    out = Buf(R, ld, C.DT[cfg["dt"]])
    ops.rows_mul(a.t, dev(inp["ra"]), b.t, dev(inp["rb"]), out.t, R=R, H=H, lda=ld, ldb=ld, ldo=ld)
    got = dict(out=out.t, guards_ok=out.guards_ok())
    settle(cfg, C.rmul_judge(cfg, inp, C.rmul_reference(cfg, inp), got), a.unchanged() and b.unchanged())


@pytest.mark.parametrize("cfg", C.bceml_cases(), ids=C.case_id)
def test_bce_multilabel_cases(cfg):
    inp = C.bceml_inputs(cfg)
    Cc, R = cfg["C"], cfg["R"]
    has = lambda name: C.bceml_has(cfg, name)                                                        # noqa: E731
    loss = torch.tensor([inp["loss0"]], dtype=torch.float32, device=DEV) if has("loss") else None
    counters = torch.full((3, Cc), inp["counters0"], dtype=torch.float32, device=DEV) if has("counters") else None
    gs_dev = scalar(inp["gs"]) if cfg["gs"] == "dev" else None
    calls, intact = [], True
    for z, y in inp["calls"]:
        zin = Buf(R, cfg["ld"], torch.float32, init=z)
        d = Buf(R, cfg["ldd"], C.DT[cfg["ddt"]]) if has("dgrad") else None
        p = Buf(R, Cc, torch.float32) if has("probs") else None
        ops.bce_multilabel(zin.t, Cc, R=R, ld=cfg["ld"], target=dev(y) if cfg["absent"] != "target" else None, pos_weight=dev(inp["pw"]), loss=loss,
                           dgrad=d.t if d else None, ldd=cfg["ldd"], grad_scale=7.0 if gs_dev is not None else inp["gs"], grad_scale_dev=gs_dev,
                           loss_scale_dev=scalar(inp["lsv"]), probs=p.t if p else None, counters=counters)
        calls.append(dict(dgrad=d.t if d else None, probs=p.t if p else None))
        intact = intact and zin.unchanged() and (d is None or d.guards_ok()) and (p is None or p.guards_ok())
    got = dict(loss=loss, counters=counters, calls=calls)
    settle(cfg, C.bceml_judge(cfg, inp, C.bceml_reference(cfg, inp), got), intact)


@pytest.mark.parametrize("cfg", C.bce_cases(), ids=C.case_id)
def test_bce_fwd_bwd_cases(cfg):
    inp = C.bce_inputs(cfg)
    A, R = cfg["A"], cfg["R"]
    has = lambda name: C.bce_has(cfg, name)                                                    # noqa: E731
    zin = Buf(R, cfg["ld"], torch.float32, init=inp["z"])
    stats = dev(inp["stats0"].copy()) if has("stats") else None
    d = Buf(R, cfg["ldd"], C.DT[cfg["ddt"]]) if has("dgrad") else None
    at = torch.full((R,), -7, dtype=torch.int64, device=DEV) if has("arg_train") else None
    ai = torch.full((R,), -7, dtype=torch.int64, device=DEV) if has("arg_infer") else None
    gs_dev = scalar(inp["gs"]) if cfg["gs"] == "dev" else None
    ops.bce_fwd_bwd(zin.t, A, R=R, ld=cfg["ld"], target=dev(inp["y"]) if cfg["absent"] != "target" else None,
                    ans_type=dev(inp["ans"]) if cfg["absent"] != "target" else None, stats=stats, dgrad=d.t if d else None, ldd=cfg["ldd"],
                    grad_scale=7.0 if gs_dev is not None else inp["gs"], grad_scale_dev=gs_dev, loss_scale_dev=scalar(inp["lsv"]),
                    arg_train=at, arg_infer=ai)
    got = dict(stats=stats, dgrad=d.t if d else None, arg_train=at, arg_infer=ai)
    settle(cfg, C.bce_judge(cfg, inp, C.bce_reference(cfg, inp), got), zin.unchanged() and (d is None or d.guards_ok()))


def _lm_fwd(cfg, inp, rows, logits, with_hit):
    """mv_lm_loss_fwd; without entry_hit through the C ABI itself (the wrapper always allocates one)"""
    n = int(inp["labels"].size)
    loss = Buf(1, max(n, 1), torch.float32)
    stat = Buf(rows, 2, torch.float32)
    hit = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV) if with_hit else None
    row_ptr, labels = dev(inp["row_ptr"]), dev(inp["labels"])
    if with_hit:
        ops.lm_loss_fwd(logits, row_ptr, labels, cfg["ls"], U=rows, V=cfg["V"], ld=cfg["ld"], entry_loss=loss.t.view(-1), entry_hit=hit, row_stat=stat.t)
    else:
        rc = ops._lib().mv_lm_loss_fwd(logits.data_ptr(), cfg["ld"], rows, cfg["V"], row_ptr.data_ptr(), labels.data_ptr() if n else None, n,
                                       float(cfg["ls"]), loss.t.data_ptr(), None, stat.t.data_ptr(), ops.L.stream_ptr())
        ops.L.check(rc, "mv_lm_loss_fwd")
    return loss, hit, stat


@pytest.mark.parametrize("cfg", C.lmf_cases(), ids=C.case_id)
def test_lm_loss_fwd_cases(cfg):
    inp = C.lmf_inputs(cfg)
    n = int(inp["labels"].size)
    zin = Buf(cfg["rows"], cfg["ld"], torch.float32, off=cfg["off"], init=inp["logits"])
    assert (zin.t.data_ptr() % 16 == 0) == (cfg["off"] == 0), cfg
    loss, hit, stat = _lm_fwd(cfg, inp, cfg["rows"], zin.t, cfg["hit"])
    got = dict(loss=loss.t.view(-1)[:n], hit=hit[:n] if hit is not None else None, stat=stat.t)
    settle(cfg, C.lmf_judge(cfg, inp, C.lmf_reference(cfg, inp), got), zin.unchanged() and stat.guards_ok() and loss.guards_ok())


@pytest.mark.parametrize("cfg", C.lms_cases(), ids=C.case_id)
def test_lm_loss_select_cases(cfg):
    inp = C.lms_inputs(cfg)
    keep, stats, inv = ops.lm_loss_select(dev(inp["loss"]), dev(inp["w"]), dev(inp["sample"]), dev(inp["hits"]), cfg["B"], cfg["k"])
    settle(cfg, C.lms_judge(cfg, inp, C.lms_reference(cfg, inp), dict(keep=keep, stats=stats, inv=inv)))


def _lm_bwd(cfg, inp, zin, stat, keep, inv):
    U = len(C.LMB_ROWS)
    d = Buf(U, cfg["ldd"], C.DT[cfg["ddt"]], off=cfg["d_off"])
    assert (zin.t.data_ptr() % 16 == 0) == (cfg["l_off"] == 0) and (d.t.data_ptr() % (4 * C.ESIZE[cfg["ddt"]]) == 0) == (cfg["d_off"] % 4 == 0), cfg
    ops.lm_loss_bwd(zin.t, dev(inp["row_ptr"]), dev(inp["labels"]), dev(inp["w"]), dev(inp["sample"]), cfg["ls"], stat, keep, inv,
                    scalar(inp["g"]), d.t, U=U, V=cfg["V"], ld=cfg["ld"], ldd=cfg["ldd"], loss_scale_dev=scalar(inp["lsv"]))
    return d


@pytest.mark.parametrize("cfg", C.lmb_cases(), ids=C.case_id)
def test_lm_loss_bwd_cases(cfg):
    inp = C.lmb_inputs(cfg)
    zin = Buf(len(C.LMB_ROWS), cfg["ld"], torch.float32, off=cfg["l_off"], init=inp["logits"])
    d = _lm_bwd(cfg, inp, zin, dev(inp["stat"]), dev(inp["keep"]), dev(inp["inv"]))
    got = dict(dlogits=d.t, guards_ok=d.guards_ok())
    settle(cfg, C.lmb_judge(cfg, inp, C.lmb_reference(cfg, inp), got), zin.unchanged())


@pytest.mark.parametrize("cfg", C.lmchain_cases(), ids=C.case_id)
def test_lm_loss_chain_cases(cfg):
    """fwd -> select -> bwd, each kernel fed by the one before it"""
    inp = C.lmchain_inputs(cfg)
    U = len(C.LMB_ROWS)
    zin = Buf(U, cfg["ld"], torch.float32, off=cfg["l_off"], init=inp["logits"])
    loss, hit, stat = _lm_fwd(cfg, inp, U, zin.t, True)
    keep, stats, inv = ops.lm_loss_select(loss.t.view(-1)[:inp["labels"].size], dev(inp["w"]), dev(inp["sample"]), hit[:inp["labels"].size],
                                          C.LMB_B, C.LMCHAIN_K)
    d = _lm_bwd(cfg, inp, zin, stat.t, keep, inv)
    got = dict(dlogits=d.t, guards_ok=d.guards_ok(), keep=keep, stats=stats)
    settle(cfg, C.lmchain_judge(cfg, inp, C.lmchain_reference(cfg, inp), got), zin.unchanged())


@pytest.mark.parametrize("cfg", C.optim_cases(), ids=C.case_id)
def test_bertadam_cases(cfg):
    """mv_tensor_sqnorms, then mv_bertadam_step, twice: each update is judged against the fp64 rule applied to the state it started from"""
    h = C.optim_hyper(cfg)
    ent, n = C.optim_layout(cfg)
    tensors, chunks = mv_optim.build_tables(ent)
    t_ref, c_ref = C.optim_tables(ent)
    assert np.array_equal(tensors.numpy(), t_ref) and np.array_equal(chunks.numpy(), c_ref), cfg
    tensors, chunks = tensors.to(DEV), chunks.to(DEV)
    host = C.optim_inputs(cfg)
    st = {k: dev(v) for k, v in host.items()}
    partials = torch.zeros(chunks.numel(), dtype=torch.float32, device=DEV)
    sq = torch.full((len(ent),), C.NAN, dtype=torch.float32, device=DEV) if cfg["mgn"] > 0 else None
    ok, worst, what = True, 0.0, []
    for k in range(2):
        step = h["first_step"] + k
        state = None
        if cfg["scaler"] != "none":                       # [3] skip flag, [4] optimizer steps applied, this one counted already
            state = torch.tensor([1024.0, 0.0, 0.0, 1.0 if cfg["scaler"] == "skip" else 0.0, float(step + 1), 0.0, 0.0, 0.0], device=DEV)
        if sq is not None:
            ops.tensor_sqnorms(st["g"], tensors, chunks, partials, sq)
        ops.bertadam_step(st["p"], st["g"], st["m"], st["v"], tensors, chunks, sq, lr=h["lr"], step=0 if cfg["scaler"] == "drive" else step,
                          warmup=h["warmup"], t_total=cfg["t_total"], schedule=cfg["sched"], b1=h["b1"], b2=h["b2"], eps=h["eps"],
                          weight_decay=h["wd"], max_grad_norm=cfg["mgn"], shadow=st["sh_bf16"], shadow_f16=st["sh_f16"], scaler_state=state)
        out = {x: st[x].cpu().numpy().copy() for x in "pgmv"}
        out.update(sh_bf16=None if st["sh_bf16"] is None else st["sh_bf16"].cpu().clone(), sh_f16=None if st["sh_f16"] is None else st["sh_f16"].cpu().clone(),
                   sq=sq.cpu().numpy() if sq is not None else None)
        o, r, w = C.optim_judge(cfg, host, C.optim_reference(cfg, host, k), out)
        ok, worst, what = ok and o, max(worst, r), what + [w] * bool(w)
        host = {x: out[x] for x in host}
    settle(cfg, (ok, worst, "; ".join(what)))


def test_worst_ratio_of_every_family():
    """(runs after the cases) the figures DESIGN.md records"""
    fams = sorted({k.split("/")[0] for k in WORST})
    print("\nworst error / bound by output encoding: " + "  ".join("%s %.4f" % (k, WORST[k]) for k in sorted(WORST)))
    print("worst error / bound: " + "  ".join("%s %.4f" % (f, max(r for k, r in WORST.items() if k.split("/")[0] == f)) for f in fams))
    assert all(r <= 1.0 for r in WORST.values())
