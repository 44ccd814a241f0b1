"""Sweep of every tile path of the attention kernels (csrc/mv_attn_mfma.hip, mv_attn_simple.hip, mv_attn_mask.hip) against fp64 references (GPU).

The cases, the dispatch restatement, the references and the bounds live in tests/attn_cases.py; tests/test_attn_cases_cpu.py counts
the paths and validates the bounds without a GPU.  Every case runs: nothing here may drop one.  Every output is pre-filled with NaN and
carries guard rows before and after; rows that are no queries, statistics beyond a sample's query count and everything past the last
packed row must come back untouched.  The backward is fed ctx and lse of the fp64 forward reference rounded to the storage types --
never the forward kernel's output -- with NaN in every row the contract says it ignores; one chained test per encoding feeds the
kernel's own forward output instead.  ctx, lse, delta, dQ, dK and dV are graded separately, per element, against
attn_cases.fwd_bounds / bwd_bounds (16-bit MFMA kernels) or the flat f32 tolerances of tests/test_kernels_gpu.py (VALU kernels).
The assertion messages carry the cfg dict, which reproduces the case.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medvill_amd import hip_ops as ops        # noqa: E402

import attn_cases as C                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = C.G_ROWS
WORST = {}


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _note(name, enc, ratio, cfg):
    key = (name, enc)
    if ratio > WORST.get(key, (-1.0, None))[0]:
        WORST[key] = (ratio, C.case_id(cfg))
    print(f"DEV attn {name} {enc} error/bound {ratio:.3e}  {C.case_id(cfg)}")


class Guarded:
    """[rows, cols] inside an allocation with G guard rows before and after, all pre-filled (NaN for floats)"""

    def __init__(self, rows, cols, dtype, fill=NAN):
        self.flat = torch.full(((rows + 2 * G), cols), fill, dtype=dtype, device=DEV)
        self.t = self.flat[G:G + rows]
        self.before = self.flat.clone()

    def guards_untouched(self):
        return _same(self.flat[:G], self.before[:G]) and _same(self.flat[G + self.t.shape[0]:], self.before[G + self.t.shape[0]:])

    def untouched(self, rows):
        """bool mask over the rows of .t: those rows kept their fill bit for bit"""
        return _same(self.t[rows], self.before[G:G + self.t.shape[0]][rows])


def _make_mask(cfg):
    """(bits int32 [B, L, W], tileinfo uint8 [B, T, T]) made by the kernel the case names"""
    B, L = cfg["B"], cfg["L"]
    W, T = (L + 31) // 32, (L + 63) // 64
    how, arg = C.mask_argument(cfg)
    bits = torch.full((B * L * W + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    info = torch.full((B * T * T + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    if how == "build":
        ops.mask_build(arg.to(DEV), B, L, bits, info)
    else:
        ops.mask_pack(arg.to(DEV), bits, info)
    return bits, info


@pytest.mark.parametrize("cfg", C.mask_cases(), ids=C.case_id)
def test_mask_bits_and_tile_classes_equal_the_restatement(cfg):
    B, L = cfg["B"], cfg["L"]
    W, T = (L + 31) // 32, (L + 63) // 64
    dense = C.dense_mask(cfg)
    bits, info = _make_mask(cfg)
    torch.cuda.synchronize()
    assert torch.equal(bits[:B * L * W].view(B, L, W).cpu(), C.pack_bits(dense)), cfg
    assert torch.equal(info[:B * T * T].view(B, T, T).cpu(), C.tile_classes(dense)), cfg
    assert bool((bits[B * L * W:] == 0x5A5A5A5A).all()) and bool((info[B * T * T:] == 0xA5).all()), cfg        # guards past W / T


def _rows_index(cfg):
    """(rowidx long [M]: logical flat position b * L + i of every existing row, in storage order; M)"""
    Lv, _, cu = C.row_plan(cfg)
    L = cfg["L"]
    idx = torch.cat([b * L + torch.arange(v) for b, v in enumerate(Lv)])
    return idx.to(DEV), int(idx.numel())


def _setup(cfg):
    enc, B, L, A, dh = cfg["enc"], cfg["B"], cfg["L"], cfg["A"], cfg["dh"]
    H = A * dh
    Lv, Lq, cu = C.row_plan(cfg)
    qkv_c, dctx_c = C.inputs(cfg)
    s = dict(enc=enc, B=B, L=L, A=A, dh=dh, H=H, Lv=Lv, Lq=Lq, dense=C.dense_mask(cfg).to(DEV), ik=C.inv_keep(cfg["p"], cfg["planes"]))
    s["qkv"], s["dctx"] = qkv_c.to(DEV), dctx_c.to(DEV)
    s["rowidx"], s["M"] = _rows_index(cfg)
    s["cu"] = torch.tensor(cu, dtype=torch.int32, device=DEV) if cu else None
    s["qlim"] = torch.tensor(cfg["qlim"], dtype=torch.int32, device=DEV) if cfg.get("qlim") else None
    pos = torch.arange(L, device=DEV).view(1, L)
    s["exist"] = (pos < torch.tensor(Lv, device=DEV).view(B, 1))                   # [B, L]
    s["query"] = (pos < torch.tensor(Lq, device=DEV).view(B, 1))
    s["bits"], s["info"] = _make_mask(cfg)
    s["keep"], s["db"] = None, None
    if cfg["p"] > 0:
        db = torch.zeros(ops.dropbits_numel(B, L, A) + 16, dtype=torch.int32, device=DEV)
        ops.attn_dropmask(cfg["p"], 0xC0FFEE + cfg["seed"], B, L, A, db, cu=s["cu"])
        s["db"], s["keep"] = db, ops.attn_keep_mask(db, B, L, A)
    s["kw"] = dict(p_drop=cfg["p"], dropbits=s["db"], cu=s["cu"], total_rows=s["M"] if cu else 0, qlim=s["qlim"])
    return s


def _packed(x, s):
    """logical [B, L, C] -> storage rows [M, C]"""
    return x.reshape(s["B"] * s["L"], -1)[s["rowidx"]]


def _logical(x, s, fill=0.0):
    out = torch.full((s["B"] * s["L"], x.shape[-1]), fill, dtype=x.dtype, device=DEV)
    out[s["rowidx"]] = x
    return out.view(s["B"], s["L"], -1)


def _knobs(cfg):
    ops.set_attn_planes(cfg["planes"])
    ops.set_attn_order(cfg["order"])
    ops.set_impl(1 if (cfg["path"] == "valu" and cfg["enc"] != C.F32) else 0)


def _restore():
    ops.set_attn_planes(16)
    ops.set_attn_order(0)
    ops.set_impl(0)


def _run_forward(cfg, s):
    B, L, A, dh, H, M = s["B"], s["L"], s["A"], s["dh"], s["H"], s["M"]
    dt = C.DT[s["enc"]]
    qkv = Guarded(M, 3 * H, dt)
    qkv.t.copy_(_packed(s["qkv"], s))
    ctx, lse = Guarded(M, H, dt), Guarded(B * A, L, torch.float32)
    ctx2 = Guarded(M, H, torch.bfloat16) if cfg["ctx2"] else None
    ops.attn_fwd(qkv.t, s["bits"], s["info"], ctx.t, lse.t, B, L, A, dh, ctx_bf16=ctx2.t if ctx2 else None, **s["kw"])
    torch.cuda.synchronize()
    return qkv, ctx, lse, ctx2


def _grade_forward(cfg, s, ctx, lse, ctx2):
    enc, B, L, A = s["enc"], s["B"], s["L"], s["A"]
    f = C.ref_forward(s["qkv"].double(), s["dense"], A, s["Lv"], s["keep"], s["ik"])
    qrow_st = _packed(s["query"].unsqueeze(-1), s).squeeze(-1)                          # query rows in storage order
    assert ctx.guards_untouched() and lse.guards_untouched(), cfg                        # nothing before the first / past the last row
    assert ctx.untouched(~qrow_st), cfg                                                  # key-only rows of ctx stay untouched
    lse_l = lse.t.view(B, A, L)
    qm = s["query"].unsqueeze(1).expand(B, A, L)
    assert _same(lse_l[~qm], torch.full_like(lse_l, NAN)[~qm]), cfg                      # no statistics beyond a sample's queries
    got = _logical(ctx.t, s)
    assert bool(torch.isfinite(got.float())[s["query"]].all()) and bool(torch.isfinite(lse_l[qm]).all()), cfg
    if cfg["path"] == "mfma":
        b_ctx, b_lse = C.fwd_bounds(f, enc, s["Lv"], s["ik"])
    else:
        dead = cfg["mask"]["kind"] == "deadrow"
        cpu = s["cpu_err"] = C.cpu_f32_errors(cfg, None if s["keep"] is None else s["keep"].cpu())
        b_ctx = C._unheads(C.flat_bound(C._heads(f["ctx"], A), enc, C.F32_TOL["ctx_dead" if dead else "ctx"], cpu["ctx"], 1e-3 * float(f["ctx"].abs().max())))
        b_lse = torch.full_like(f["lse"], max(C.F32_TOL["lse_dead" if dead else "lse"], 4.0 * cpu["lse"]))
    r_ctx, i_ctx = C.worst_ratio(got, f["ctx"], b_ctx, s["query"].unsqueeze(-1))
    r_lse, i_lse = C.worst_ratio(lse_l, f["lse"], b_lse, qm)
    _note("ctx", enc + ("" if cfg["path"] == "mfma" else "-valu"), r_ctx, cfg)
    _note("lse", enc + ("" if cfg["path"] == "mfma" else "-valu"), r_lse, cfg)
    assert r_ctx <= 1.0, (cfg, "ctx", r_ctx, i_ctx)
    assert r_lse <= 1.0, (cfg, "lse", r_lse, i_lse)
    if ctx2 is not None:           # the bf16 copy: the same accumulator rounded to bf16, so within one bf16 ulp of the f16 value
        assert ctx2.guards_untouched() and ctx2.untouched(~qrow_st), cfg
        a, b = ctx2.t[qrow_st].double(), ctx.t[qrow_st].double()
        assert bool(((a - b).abs() <= 2.0 ** -7 * b.abs() + 2.0 ** -24).all()), cfg
        assert C.worst_ratio(_logical(ctx2.t, s), f["ctx"], C.fwd_bounds(f, enc, s["Lv"], s["ik"], store=C.BF16)[0], s["query"].unsqueeze(-1))[0] <= 1.0, cfg
    return f


def _run_backward(cfg, s, ctx_in, lse_in):
    """ctx_in [B, L, H] in the encoding and lse_in f32 [B, A, L] (logical); rows the contract ignores are fed NaN"""
    B, L, A, dh, H, M = s["B"], s["L"], s["A"], s["dh"], s["H"], s["M"]
    dt = C.DT[s["enc"]]
    nanrow = ~s["query"].unsqueeze(-1)
    qkv = Guarded(M, 3 * H, dt)
    qkv.t.copy_(_packed(s["qkv"], s))
    mfma = cfg["path"] == "mfma"
    ctx_f = torch.where(nanrow, torch.full_like(ctx_in, NAN), ctx_in) if mfma else ctx_in
    dctx_f = torch.where(nanrow, torch.full_like(s["dctx"], NAN), s["dctx"]) if mfma else s["dctx"]
    lse_f = torch.where(s["query"].unsqueeze(1), lse_in, torch.full_like(lse_in, NAN)) if mfma else lse_in
    ctxg, dctxg = Guarded(M, H, dt), Guarded(M, H, dt)
    ctxg.t.copy_(_packed(ctx_f, s))
    dctxg.t.copy_(_packed(dctx_f, s))
    dqkv, delta = Guarded(M, 3 * H, dt), Guarded(B * A, L, torch.float32)
    ops.attn_bwd(qkv.t, ctxg.t, dctxg.t, lse_f.contiguous().view(B * A, L), s["bits"], s["info"], dqkv.t, delta.t, B, L, A, dh, **s["kw"])
    torch.cuda.synchronize()
    return dqkv, delta


def _grade_backward(cfg, s, ctx_in, lse_in, dqkv, delta, tag=""):
    enc, B, L, A, H = s["enc"], s["B"], s["L"], s["A"], s["H"]
    r = C.ref_backward(s["qkv"].double(), ctx_in.double(), s["dctx"].double(), lse_in.double(), s["dense"], A, s["Lv"], s["Lq"], s["keep"], s["ik"])
    assert dqkv.guards_untouched() and delta.guards_untouched(), cfg                     # nothing is written past cu[B]
    assert bool(torch.isfinite(dqkv.t.float()).all()), cfg                               # every existing row is written
    got = _logical(dqkv.t, s)
    dl = delta.t.view(B, A, L)
    qm = s["query"].unsqueeze(1).expand(B, A, L)
    if cfg["path"] == "mfma":
        assert _same(dl[~qm], torch.full_like(dl, NAN)[~qm]), cfg
        keyonly = (s["exist"] & ~s["query"]).unsqueeze(-1)
        assert bool((torch.where(keyonly, got[..., :H].float(), torch.zeros((), device=DEV)) == 0).all()), cfg    # zero dQ rows for key-only rows
        bb = C.bwd_bounds(r, enc, s["Lv"], s["ik"])
    else:
        dead = cfg["mask"]["kind"] == "deadrow"
        tol = C.F32_TOL["grad_dead" if dead else "grad"]
        floor = 1e-3 * max(float(r[n].abs().max()) for n in ("dq", "dk", "dv"))
        # the flat tolerance per row, plus the f32 first-order terms: a row whose exact gradient is zero (one visible key) still carries
        # the cancellation error of dP - delta
        arith = C.bwd_bounds(r, C.F32, s["Lv"], s["ik"])
        bb = {n: C._unheads(C.flat_bound(C._heads(r[n], A), enc, tol, s["cpu_err"]["grad"], floor)) + arith[n] for n in ("dq", "dk", "dv")}
        bb["delta"] = arith["delta"]
    name_enc = enc + tag + ("" if cfg["path"] == "mfma" else "-valu")
    for i, n in enumerate(("dq", "dk", "dv")):
        ratio, at = C.worst_ratio(got[..., i * H:(i + 1) * H], r[n], bb[n], s["exist"].unsqueeze(-1))
        _note(n, name_enc, ratio, cfg)
        assert ratio <= 1.0, (cfg, n, ratio, at)
    ratio, at = C.worst_ratio(dl, r["delta"], bb["delta"], qm)
    _note("delta", name_enc, ratio, cfg)
    assert ratio <= 1.0, (cfg, "delta", ratio, at)


def _forward_and_backward(cfg):
    try:
        _knobs(cfg)
        s = _setup(cfg)
        qkv, ctx, lse, ctx2 = _run_forward(cfg, s)
        assert _same(qkv.flat[G:G + s["M"]], _packed(s["qkv"], s)), cfg
        f = _grade_forward(cfg, s, ctx, lse, ctx2)
        ctx_in, lse_in = f["ctx"].to(C.DT[s["enc"]]), f["lse"].float()
        dqkv, delta = _run_backward(cfg, s, ctx_in, lse_in)
        _grade_backward(cfg, s, ctx_in, lse_in, dqkv, delta)
        if cfg["order"] == 1:            # placement is a speed matter only: bit-identical outputs in both orders
            ops.set_attn_order(0)
            _, ctx0, lse0, _ = _run_forward(cfg, s)
            dqkv0, delta0 = _run_backward(cfg, s, ctx_in, lse_in)
            assert _same(ctx0.flat, ctx.flat) and _same(lse0.flat, lse.flat) and _same(dqkv0.flat, dqkv.flat) and _same(delta0.flat, delta.flat), cfg
    finally:
        _restore()


@pytest.mark.parametrize("cfg", C.mfma_cases(), ids=C.case_id)
def test_family_masks_every_length_plan_and_value_set(cfg):
    _forward_and_backward(cfg)


@pytest.mark.parametrize("cfg", C.dense_cases(), ids=C.case_id)
def test_dense_masks_holes_split_classes_dead_rows_ragged_ones(cfg):
    _forward_and_backward(cfg)


@pytest.mark.parametrize("cfg", C.knob_cases(), ids=C.case_id)
def test_dropout_plane_counts_and_block_order_1(cfg):
    _forward_and_backward(cfg)


@pytest.mark.parametrize("cfg", C.valu_cases(), ids=C.case_id)
def test_valu_kernels_every_dh_and_encoding(cfg):
    _forward_and_backward(cfg)


@pytest.mark.parametrize("cfg", [C.mfma_case(13), C.mfma_case(17), C.dense_case(9), C.dense_case(3)], ids=C.case_id)
def test_chained_backward_on_the_forward_kernels_own_output(cfg):
    """as the model runs them: the backward reads the forward kernel's ctx and lse; graded against the contract evaluated at those"""
    try:
        _knobs(cfg)
        s = _setup(cfg)
        _, ctx, lse, _ = _run_forward(cfg, s)
        ctx_in = torch.nan_to_num(_logical(ctx.t, s))
        lse_in = torch.nan_to_num(lse.t.view(s["B"], s["A"], s["L"]))
        dqkv, delta = _run_backward(cfg, s, ctx_in, lse_in)
        _grade_backward(cfg, s, ctx_in, lse_in, dqkv, delta, tag="-chained")
    finally:
        _restore()


@pytest.mark.parametrize("planes", C.PLANES)
@pytest.mark.parametrize("B,L,A,lens", [(2, 193, 3, [65, 193]), (3, 321, 2, [1, 128, 300]), (1, 64, 1, [33]), (1, 256, 2, [200]), (2, 256, 1, [33, 256])])
def test_dropmask_words_fraction_independence_and_packed_equals_padded(planes, B, L, A, lens):
    try:
        ops.set_attn_planes(planes)
        p, key = 0.1, 0xABCDEF0123
        n = ops.dropbits_numel(B, L, A)
        nblocks = (n // 2 + 255) // 256
        remap = C.dropmask_block_map(nblocks, B * A)           # L = 256 with two pairs: 4 blocks per pair, the spread order; the others: identity
        assert (remap != list(range(nblocks))) == (L == 256) and sorted(remap) == list(range(nblocks))
        fill = 0x3C3C3C3C
        pad, pk, other = (torch.full((n + 16,), fill, dtype=torch.int32, device=DEV) for _ in range(3))
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        ops.attn_dropmask(p, key, B, L, A, pad)
        ops.attn_dropmask(p, key, B, L, A, pk, cu=cu)
        ops.attn_dropmask(p, key + 1, B, L, A, other)
        torch.cuda.synchronize()
        assert all(bool((t[n:] == fill).all()) for t in (pad, pk, other))
        NQB, NKT = (L + 31) // 32, (L + 63) // 64
        blocks = pk[:n].view(B, A, NQB, NKT, 64)
        qb = torch.arange(NQB, device=DEV).view(1, 1, NQB, 1) * 32
        kt = torch.arange(NKT, device=DEV).view(1, 1, 1, NKT) * 64
        lv = torch.tensor(lens, device=DEV).view(B, 1, 1, 1)
        live = ((qb < lv) & (kt < lv)).expand(B, A, NQB, NKT)
        assert bool((blocks[~live] == fill).all())                                    # untouched exactly where no query or key exists
        assert torch.equal(blocks[live], pad[:n].view(B, A, NQB, NKT, 64)[live])      # ... and the padded run's words everywhere else
        keep, k2 = ops.attn_keep_mask(pad, B, L, A).double(), ops.attn_keep_mask(other, B, L, A).double()
        want = 1.0 - C.drop_thr(p, planes) / float(1 << planes)
        sigma = math.sqrt(want * (1 - want) / keep.numel())
        assert abs(float(keep.mean()) - want) < 5 * sigma, (planes, float(keep.mean()), want)
        assert abs(float(k2.mean()) - want) < 5 * sigma
        assert abs(float((keep * k2).mean()) - want * want) < 5 * math.sqrt(want * want * (1 - want * want) / keep.numel()) + 10 * sigma * want
        assert abs(C.inv_keep(p, planes) * want - 1.0) < 1e-6
    finally:
        _restore()


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module's tests: per output and encoding, the worst error / bound of whatever ran (the figures DESIGN.md records)"""
    yield
    for key in sorted(WORST):
        print(f"WORST {key[0]:6s} {key[1]:18s} {WORST[key][0]:.3f}   {WORST[key][1]}")
