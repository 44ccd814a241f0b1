"""Case generator, dispatch restatement, fp64 references and bounds of the embedding sweep (embed_fwd_kernel / embed_bwd_kernel of
csrc/mv_rowops.hip, behind mv_embed_fwd / mv_embed_bwd).

Plain module in the style of rowops_cases.py, whose encodings, bounds and dropout restatement it reuses: nothing here touches the GPU or
the HIP library.  tests/test_wave_per_row_embed_sweep_gpu.py (both are one-wave-per-row kernels) runs the cases on the kernels;
tests/test_embed_cases_cpu.py counts the branches, pins the constants to the source, and runs the very same checks on a plain f32 torch
implementation, so that no bound is tuned to the kernels.

* a case is a dict drawn from np.random.RandomState(fixed + seed); ids, packed rows and tensors are made from the cfg alone;
* emb_branches restates what both launchers and emb_decode do with a case, for the census;
* emb_reference is plain torch in fp64 with autograd; emb_reference_closed_form is a second formulation of the backward;
* check_forward / check_backward hold every assertion on a set of outputs, wherever those outputs come from.
"""
import numpy as np
import torch
import torch.nn.functional as F

from rowops_cases import (BF16, DT, F16, F32, LN_MAX_H, LN_NC_STEPS, U32, dm_restated, dm_threshold, ln_bwd_closed_form, ln_case_tol,
                          ln_nc, ln_term_errors, out16_bound, rowrel, sum_bound)

# ---- constants of the launchers (tests/test_embed_cases_cpu.py reads the same numbers out of the source) ---------------------------
EMB_MAX_H = LN_MAX_H
EMB_NC_STEPS = LN_NC_STEPS           # mv_with_row_chunks: 1, 3, 4 chunks of 256 columns up to these widths, else 8
EMB_BWD_BLOCKS = 1024                # mv_embed_bwd: at most this many blocks; beyond it a wave walks several rows
EMB_ROWS_PER_BLOCK = 4               # one wave per row, four waves per block, in both kernels
EMB_HOT_TOKEN = 103                  # MV_HOT_TOKEN: the id whose look-up gradient is summed per block
EMB_FWD_TOL, EMB_BWD_TOL = 1e-5, 1e-4      # the f32 tolerances of tests/test_kernels_gpu.py and of the LayerNorm sweep, row-relative
EMB_MEAN_TOL, EMB_RSTD_TOL = 1e-5, 1e-4    # mean against the row's largest |pre|, rstd relative: as the LayerNorm forward sweep

EMB_H = (4, 132, 256, 260, 764, 768, 1024, 1028, 2044, 2048)
EMB_SHAPES = ((1, 0, 1), (2, 1, 3), (3, 5, 30), (5, 36, 27))          # (B, N, T)
EMB_DROP = ((0.0, 0.0), (0.1, 0.1), (0.1, 0.5))                       # (text rows, image rows)
EMB_UNSCALE = (None, 0.25, 1.0 / 1024)
EMB_PAD = (0, -1, 103)
EMB_V = (50, 104, 1000)
EMB_MAXPOS = (1, 40, 64, 512)                                         # maxpos = max(T, one of these)
EMB_EPS = (1e-12, 1e-5)
EMB_ROWMAPS = ("none", "prefix", "perm")
BAD_TOK_NEG = (-1, -5, -2 ** 31)
BAD_SEG = (-1, 2, 7)
N_EMB = 64


def BAD_TOK_HIGH(V):
    return (V, V + 7, 2 ** 31 - 1)


def BAD_POS(maxpos):
    return (-3, maxpos, maxpos + 9)


def emb_case(seed):
    rs = np.random.RandomState(7700 + seed)
    B, N, T = EMB_SHAPES[int(rs.choice(4, p=[0.1, 0.2, 0.35, 0.35]))]
    dt = (F32, BF16, F16)[seed % 3]
    p_drop, p_drop_img = EMB_DROP[int(rs.randint(3))]
    return dict(fam="emb", seed=seed, H=int(EMB_H[seed % len(EMB_H)]), dt=dt, x0_bf16=bool(dt == F16 and rs.randint(2)), B=B, N=N, T=T,
                img_pos=bool(N > 0 and rs.randint(3) > 0), rowmap=EMB_ROWMAPS[(seed // 3) % 3], min_len=1, eps=float(rs.choice(EMB_EPS)),
                p_drop=p_drop, p_drop_img=p_drop_img, drop_key=int(rs.randint(1, 2 ** 31)) * 2654435761 % 2 ** 63,
                unscale=EMB_UNSCALE[int(rs.randint(3))], pad=int(EMB_PAD[int(rs.randint(3))]), V=int(EMB_V[int(rs.randint(3))]),
                maxpos=max(T, int(rs.choice(EMB_MAXPOS))), bad=bool(seed % 4 == 1 or seed % 16 == 2))


EMB_FIXED = [
    # the backward's row walk: more rows than 1024 blocks x 4 waves, so the register accumulators carry over from row to row
    dict(fam="emb", seed=9701, H=132, dt=F32, x0_bf16=False, B=33, N=60, T=64, img_pos=True, rowmap="none", min_len=1, eps=1e-12, p_drop=0.1,
         p_drop_img=0.5, drop_key=0x0123456789abcdef, unscale=0.25, pad=0, V=1000, maxpos=512, bad=True),
    # the same walk over packed rows
    dict(fam="emb", seed=9702, H=132, dt=F16, x0_bf16=True, B=40, N=60, T=64, img_pos=True, rowmap="prefix", min_len=110, eps=1e-12,
         p_drop=0.1, p_drop_img=0.1, drop_key=77, unscale=1.0 / 1024, pad=-1, V=1000, maxpos=64, bad=True),
    # BERT-base's own row: three chunks of 256 columns, bf16, packed rows, dropout and unscale; enough rows for the walk
    dict(fam="emb", seed=9703, H=768, dt=BF16, x0_bf16=False, B=40, N=60, T=64, img_pos=True, rowmap="prefix", min_len=105, eps=1e-12,
         p_drop=0.1, p_drop_img=0.1, drop_key=20240607, unscale=1.0 / 1024, pad=0, V=1000, maxpos=512, bad=False),
    # BERT-base's row at a batch the CPU can check as well, permuted rows
    dict(fam="emb", seed=9704, H=768, dt=BF16, x0_bf16=False, B=5, N=36, T=27, img_pos=True, rowmap="perm", min_len=1, eps=1e-12,
         p_drop=0.1, p_drop_img=0.5, drop_key=99, unscale=0.25, pad=0, V=1000, maxpos=512, bad=True),
    # f16 with its bf16 shadow over eight chunks, the last one ragged
    dict(fam="emb", seed=9705, H=2044, dt=F16, x0_bf16=True, B=3, N=5, T=30, img_pos=False, rowmap="perm", min_len=1, eps=1e-5,
         p_drop=0.1, p_drop_img=0.5, drop_key=5, unscale=None, pad=103, V=104, maxpos=30, bad=True),
]


def emb_cases():
    return [emb_case(s) for s in range(N_EMB)] + EMB_FIXED


def emb_L(cfg):
    return cfg["N"] + cfg["T"] + 2


def emb_rowmap(cfg):
    """The packed rows of a case: None, or int32 [n_rows] of distinct logical rows b * L + l.  "prefix": the first len_b positions of every
    sample in ascending order, as the engine's padding removal produces them; "perm": one permuted subset of all rows."""
    if cfg["rowmap"] == "none":
        return None
    B, L = cfg["B"], emb_L(cfg)
    rs = np.random.RandomState(7800 + cfg["seed"])
    if cfg["rowmap"] == "prefix":
        lens = rs.randint(min(cfg["min_len"], L), L + 1, size=B)
        return np.concatenate([b * L + np.arange(n) for b, n in enumerate(lens)]).astype(np.int32)
    k = int(rs.randint(max(1, (B * L) // 2), B * L + 1))
    return rs.permutation(B * L)[:k].astype(np.int32)


def emb_n_rows(cfg):
    rm = emb_rowmap(cfg)
    return cfg["B"] * emb_L(cfg) if rm is None else len(rm)


def emb_ids(cfg):
    """int64 numpy arrays cls [B], sep [B], txt [B, T], seg [B, T], img_pos [B, N] or None.  The text draws from a small pool (repeated
    ids), carries a run of id 103 and ends in pad ids; the bad flavour plants ids outside every table.  Negative token ids go to samples
    b >= 1 of cases with N >= 1 only: there even a kernel that took -1 for an image region would stay inside imgproj and dimg."""
    B, N, T, V, maxpos, pad = cfg["B"], cfg["N"], cfg["T"], cfg["V"], cfg["maxpos"], cfg["pad"]
    rs = np.random.RandomState(7750 + cfg["seed"])
    cls, sep = np.full(B, 101, dtype=np.int64), np.full(B, 102, dtype=np.int64)
    pool = rs.randint(0, V, size=max(2, T // 2)).astype(np.int64)
    txt = pool[rs.randint(len(pool), size=(B, T))]
    if T >= 4:
        k = max(1, T // 5)
        txt[:, 1:1 + k] = EMB_HOT_TOKEN
        txt[:, T - k:] = pad if pad >= 0 else 0
        txt[:, T - k - 1] = 0                       # id 0 occurs whatever the pad id is
    seg = rs.randint(0, 2, size=(B, T)).astype(np.int64)
    img_pos = None
    if cfg["img_pos"] and N > 0:
        img_pos = np.stack([np.sort(rs.randint(0, maxpos, size=N)) for _ in range(B)]).astype(np.int64)
    if cfg["bad"]:
        k = min(T, 3)
        txt[0, :k] = BAD_TOK_HIGH(V)[:k]
        seg[B - 1, T - k:] = BAD_SEG[:k]
        if B >= 2 and N >= 1:
            txt[1, :k] = BAD_TOK_NEG[:k]
            cls[1], sep[B - 1] = -1, -5
            if B >= 3:
                cls[2], sep[1] = -2 ** 31, -1
        if img_pos is not None:
            k = min(img_pos.size, 3)
            img_pos.reshape(-1)[:k] = BAD_POS(maxpos)[:k]
    return dict(cls=cls, sep=sep, txt=txt, seg=seg, img_pos=img_pos)


def c_int(a):
    """(int) of an int64, as emb_decode casts every id: the low 32 bits, signed"""
    return np.asarray(a, dtype=np.int64).astype(np.int32).astype(np.int64)


def emb_decode_host(cfg, ids, li):
    """emb_decode of csrc/mv_rowops.hip for an array of logical rows li = b * L + l -> (tok, pos, typ, reg, b), int64 arrays.
    tok == -1 and reg >= 0: an image region (l in 1..N), and only that.  A token id >= V reads row V - 1, a negative one row 0; a
    position outside 0..maxpos-1 and a type outside 0..1 go to the nearer end.  pos == -1: no position embedding (image rows of a case
    without img_pos)."""
    N, T, V, maxpos, L = cfg["N"], cfg["T"], cfg["V"], cfg["maxpos"], emb_L(cfg)
    li = np.asarray(li, dtype=np.int64)
    b, l = li // L, li % L
    tok, pos, typ, reg = (np.zeros(len(li), dtype=np.int64) for _ in range(4))
    reg[:] = -1
    m_cls, m_img, m_sep, m_txt = l == 0, (l >= 1) & (l <= N), l == N + 1, l > N + 1
    tok[m_cls] = c_int(ids["cls"][b[m_cls]])
    tok[m_sep] = c_int(ids["sep"][b[m_sep]])
    t = l[m_txt] - N - 2
    tok[m_txt], pos[m_txt], typ[m_txt] = c_int(ids["txt"][b[m_txt], t]), t, c_int(ids["seg"][b[m_txt], t])
    reg[m_img] = l[m_img] - 1
    tok[m_img] = -1
    if ids["img_pos"] is not None:
        pos[m_img] = c_int(ids["img_pos"][b[m_img], reg[m_img]])
    tok = np.where(tok >= V, V - 1, tok)
    tok = np.where(~m_img & (tok < 0), 0, tok)
    pos = np.clip(pos, 0, maxpos - 1)
    if ids["img_pos"] is None:
        pos[m_img] = -1
    return tok, pos, np.clip(typ, 0, 1), reg, b


def emb_raw_rows(cfg, ids, li):
    """The ids as the case holds them, before any clamp, per mapped row li -> (token id, image position, segment, image-row mask,
    sample); a field a row does not have (the token of an image row, the segment of [CLS]) is 0."""
    N, L = cfg["N"], emb_L(cfg)
    li = np.asarray(li, dtype=np.int64)
    b, l = li // L, li % L
    m_cls, m_img, m_sep, m_txt = l == 0, (l >= 1) & (l <= N), l == N + 1, l > N + 1
    tok = np.zeros(len(li), dtype=np.int64)
    tok[m_cls], tok[m_sep] = ids["cls"][b[m_cls]], ids["sep"][b[m_sep]]
    tok[m_txt] = ids["txt"][b[m_txt], l[m_txt] - N - 2]
    seg = np.zeros(len(li), dtype=np.int64)
    seg[m_txt] = ids["seg"][b[m_txt], l[m_txt] - N - 2]
    pos = np.zeros(len(li), dtype=np.int64)
    if ids["img_pos"] is not None:
        pos[m_img] = ids["img_pos"][b[m_img], l[m_img] - 1]
    return tok, pos, seg, m_img, b


def emb_branches(cfg):
    """What a case takes through mv_embed_fwd, mv_embed_bwd and emb_decode, by name (for the census).  Everything about ids counts the
    rows that reach the kernels only: a planted id in a row the packed rows leave out names nothing."""
    H, V, pad = cfg["H"], cfg["V"], cfg["pad"]
    ids, rm = emb_ids(cfg), emb_rowmap(cfg)
    n_rows = emb_n_rows(cfg)
    li = np.arange(n_rows) if rm is None else rm
    nc = ln_nc(H)
    b = [f"nc{nc}", f"dt_{cfg['dt']}", f"rowmap_{cfg['rowmap']}", f"n_rows%4={n_rows % 4}"]
    if H % 256 and nc > 1:
        b.append("ragged_chunk")
    if cfg["x0_bf16"]:
        b.append("x0_bf16")
    if n_rows > EMB_BWD_BLOCKS * EMB_ROWS_PER_BLOCK:
        b.append("bwd_row_walk")
    if cfg["N"] == 0:
        b.append("N=0")
    elif not cfg["img_pos"]:
        b.append("img_pos_none")
    b.append("drop_%g_%g" % (cfg["p_drop"], cfg["p_drop_img"]))
    b.append("unscale_none" if cfg["unscale"] is None else "unscale_%g" % cfg["unscale"])
    b.append("pad_%d" % pad)
    if EMB_HOT_TOKEN >= V:
        b.append("hot>=V")
    if EMB_HOT_TOKEN == V - 1:
        b.append("hot==V-1")
    tok, pos, typ, reg, _ = emb_decode_host(cfg, ids, li)
    if bool(((tok == EMB_HOT_TOKEN) & (reg < 0)).any()):
        b.append("hot_rows")
    raw_tok, raw_pos, raw_seg, m_img, smp = emb_raw_rows(cfg, ids, li)
    if bool((~m_img & (raw_tok >= V)).any()):
        b.append("bad_tok_high")
    if bool((~m_img & (raw_tok == -1)).any()):
        b.append("bad_tok_neg1")
    if bool((~m_img & (raw_tok < -1)).any()):
        b.append("bad_tok_below_neg1")
    if ids["img_pos"] is not None and bool((m_img & ((raw_pos < 0) | (raw_pos >= cfg["maxpos"]))).any()):
        b.append("bad_pos")
    if bool((~m_img & ((raw_seg < 0) | (raw_seg > 1))).any()):
        b.append("bad_seg")
    return b


def emb_census():
    count = {}
    for c in emb_cases():
        for name in emb_branches(c):
            count[name] = count.get(name, 0) + 1
    return count


# =====================================================================================================================
# inputs
# =====================================================================================================================
ACC = ("dE", "dP", "dTy", "dg", "db")          # the five f32 accumulators of the backward


def emb_inputs(cfg):
    """CPU tensors of a case, from cfg["seed"] alone: ids (int64), rowmap (int32 or None), the tables and imgproj in the case's encoding
    (about 0.05 randn and 0.5 randn), gamma = 1 + 0.1 randn, beta = 0.1 randn, the incoming gradient dx0 [n_rows, H] in the encoding, and
    "prev": what the five f32 accumulators hold before the backward (a random, non-zero previous gradient)."""
    B, N, T, H, V, maxpos = cfg["B"], cfg["N"], cfg["T"], cfg["H"], cfg["V"], cfg["maxpos"]
    g = torch.Generator().manual_seed(cfg["seed"])
    dt = DT[cfg["dt"]]

    def rn(shape, scale):
        return torch.randn(shape, generator=g) * scale
    ids, rm = emb_ids(cfg), emb_rowmap(cfg)
    n_rows = emb_n_rows(cfg)
    inp = dict(n_rows=n_rows, ids=ids, rowmap_np=rm, rowmap=None if rm is None else torch.from_numpy(rm),
               cls=torch.from_numpy(ids["cls"]), sep=torch.from_numpy(ids["sep"]), txt=torch.from_numpy(ids["txt"]),
               seg=torch.from_numpy(ids["seg"]), img_pos=None if ids["img_pos"] is None else torch.from_numpy(ids["img_pos"]))
    inp["E"], inp["P"], inp["Ty"] = rn((V, H), 0.05).to(dt), rn((maxpos, H), 0.05).to(dt), rn((2, H), 0.05).to(dt)
    inp["imgproj"] = rn((B * N, H), 0.5).to(dt) if N else None
    inp["gamma"], inp["beta"] = 1.0 + rn((H,), 0.1), rn((H,), 0.1)
    inp["dx0"] = rn((n_rows, H), 1.0).to(dt)
    inp["prev"] = dict(dE=rn((V, H), 0.05), dP=rn((maxpos, H), 0.05), dTy=rn((2, H), 0.05), dg=rn((H,), 0.05), db=rn((H,), 0.05))
    return inp


def emb_keep(cfg, is_img, n_rows):
    """The dropout of both kernels: element c of PACKED row r is kept when its 16-bit hash half at element index r * H + c is not
    below the threshold of its row kind (text and image rows have their own); survivors are scaled by 65536 / (65536 - thr).
    is_img: bool numpy [n_rows].  -> (keep bool numpy [n_rows, H], scale float64 numpy [n_rows, 1])"""
    H = cfg["H"]
    kt = dm_restated(cfg["p_drop"], cfg["drop_key"], n_rows * H).reshape(n_rows, H).astype(bool)
    ki = dm_restated(cfg["p_drop_img"], cfg["drop_key"], n_rows * H).reshape(n_rows, H).astype(bool)
    thr = np.where(is_img, dm_threshold(cfg["p_drop_img"]), dm_threshold(cfg["p_drop"])).astype(np.float64)
    return np.where(is_img[:, None], ki, kt), (65536.0 / (65536.0 - thr))[:, None]


# =====================================================================================================================
# references
# =====================================================================================================================
def emb_reference(cfg, inp, device="cpu"):
    """Both kernels in fp64 torch, the backward by autograd: positions decoded on the host with the documented clamps,
    pre = (E | imgproj)[..] + P[..] + Ty[..] (no P term on image rows without img_pos), F.layer_norm, dropout by the restated mask at
    element index packed_row * H + c, F.embedding(padding_idx = pad) semantics for the look-up gradient.  Everything is in packed row
    order.  Also returns pre_f32: (e.float() + p.float()) + t.float(), the f32 expression the forward kernel evaluates."""
    H, V, N, pad, eps, n = cfg["H"], cfg["V"], cfg["N"], cfg["pad"], cfg["eps"], inp["n_rows"]
    dev = torch.device(device)
    li = np.arange(n) if inp["rowmap_np"] is None else inp["rowmap_np"]
    tok_n, pos_n, typ_n, reg_n, b_n = emb_decode_host(cfg, inp["ids"], li)
    tok, pos, typ, reg, b = (torch.from_numpy(a).to(dev) for a in (tok_n, pos_n, typ_n, reg_n, b_n))
    is_img, haspos = reg >= 0, pos >= 0
    raw = {k: inp[k].to(dev) for k in ("E", "P", "Ty")}
    E, P, Ty = (raw[k].double().requires_grad_(True) for k in ("E", "P", "Ty"))
    gamma, beta = (inp[k].to(dev).double().requires_grad_(True) for k in ("gamma", "beta"))
    tok_c, pos_c = tok.clamp(min=0), pos.clamp(min=0)
    e = F.embedding(tok_c, E, padding_idx=pad if 0 <= pad < V else None)
    e32 = raw["E"][tok_c].float()
    img = None
    if N:
        img_raw = inp["imgproj"].to(dev)
        img = img_raw.double().requires_grad_(True)
        region = (b * N + reg.clamp(min=0))
        e = torch.where(is_img[:, None], img[region], e)
        e32 = torch.where(is_img[:, None], img_raw[region].float(), e32)
    pre = e + P[pos_c] * haspos[:, None] + Ty[typ]
    pre.retain_grad()
    pre_f32 = torch.where(haspos[:, None], (e32 + raw["P"][pos_c].float()) + raw["Ty"][typ].float(), e32 + raw["Ty"][typ].float())
    y = F.layer_norm(pre, (H,), gamma, beta, eps)
    keep_n, scale_n = emb_keep(cfg, reg_n >= 0, n)
    keep, scale = torch.from_numpy(keep_n).to(dev), torch.from_numpy(scale_n).to(dev)
    x0 = y * keep * scale
    dx0 = inp["dx0"].to(dev).double()
    (x0 * dx0).sum().backward()
    pre_d = pre.detach()
    mean = pre_d.mean(dim=1)
    rstd = 1.0 / torch.sqrt(pre_d.var(dim=1, unbiased=False) + eps)
    return dict(n_rows=n, tok=tok, pos=pos, typ=typ, reg=reg, b=b, is_img=is_img, haspos=haspos, pre=pre_d, pre_f32=pre_f32, y=y.detach(),
                keep=keep, scale=scale, x0=x0.detach(), mean=mean, rstd=rstd, xhat=(pre_d - mean[:, None]) * rstd[:, None],
                d=dx0 * keep * scale, dpre=pre.grad, dE=E.grad, dP=P.grad, dTy=Ty.grad, dg=gamma.grad, db=beta.grad,
                dimg=None if img is None else img.grad)


def emb_scatter_plan(cfg, ref):
    """which packed rows add into which row of the three tables: name -> (row index per packed row, bool mask of the rows that add)"""
    pad = cfg["pad"]
    every = torch.ones_like(ref["is_img"])
    return {"dE": (ref["tok"].clamp(min=0), ~ref["is_img"] & (ref["tok"] != pad)), "dP": (ref["pos"].clamp(min=0), ref["haspos"]),
            "dTy": (ref["typ"], every)}


def emb_reference_closed_form(cfg, inp, ref):
    """The backward a second time, without autograd and without F.embedding: the closed form of the LayerNorm backward
    (rowops_cases.ln_bwd_closed_form) on the row sums built by plain indexing, then index_add_ into zeroed tables."""
    H, N = cfg["H"], cfg["N"]
    dev = ref["pre"].device
    E, P, Ty = (inp[k].to(dev).double() for k in ("E", "P", "Ty"))
    pre = E[ref["tok"].clamp(min=0)]
    if N:
        img = inp["imgproj"].to(dev).double()[ref["b"] * N + ref["reg"].clamp(min=0)]
        pre = torch.where(ref["is_img"][:, None], img, pre)
    pre = pre + torch.where(ref["haspos"][:, None], P[ref["pos"].clamp(min=0)], torch.zeros_like(pre)) + Ty[ref["typ"]]
    d = inp["dx0"].to(dev).double() * ref["keep"] * ref["scale"]
    dpre, dgamma, dbeta = ln_bwd_closed_form(pre, inp["gamma"].to(dev).double(), d, cfg["eps"])
    out = dict(pre=pre, dpre=dpre, dg=dgamma, db=dbeta)
    for name, (idx, mask) in emb_scatter_plan(cfg, ref).items():
        t = torch.zeros_like(inp["prev"][name], dtype=torch.float64, device=dev)
        out[name] = t.index_add_(0, idx[mask], dpre[mask])
    if N:
        out["dimg"] = torch.zeros((cfg["B"] * N, H), dtype=torch.float64, device=dev)
        out["dimg"][(ref["b"] * N + ref["reg"])[ref["is_img"]]] = dpre[ref["is_img"]]
    return out


def emb_f32_cpu(cfg, inp, ref):
    """F.layer_norm and its autograd in plain f32 on the CPU on the case's own pre and incoming gradient: what the f32 tolerances of a
    case are measured from (rowops_cases.ln_case_tol), never from the code under test.  -> (y, dpre), f32 CPU tensors"""
    pre = ref["pre_f32"].cpu().clone().requires_grad_(True)
    H = pre.shape[1]
    y = F.layer_norm(pre, (H,), inp["gamma"].float().cpu(), inp["beta"].float().cpu(), cfg["eps"])
    (y * ref["d"].float().cpu()).sum().backward()
    return y.detach(), pre.grad


def emb_tolerances(cfg, inp, ref):
    """(forward tolerance, backward tolerance of the image rows) of a case, row-relative: ln_case_tol over plain f32 torch on the CPU"""
    y_cpu, dpre_cpu = emb_f32_cpu(cfg, inp, ref)
    dev = ref["pre"].device
    fwd = ln_case_tol(EMB_FWD_TOL, y_cpu.to(dev), ref["y"])
    img = ref["is_img"]
    bwd = ln_case_tol(EMB_BWD_TOL, dpre_cpu.to(dev)[img], ref["dpre"][img]) if bool(img.any()) else EMB_BWD_TOL
    return fwd, bwd


# =====================================================================================================================
# the checks (on the outputs of the kernels, or of anything else that claims to compute the same)
# =====================================================================================================================
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _within(got, ref, bound):
    r = ((got.double() - ref).abs() / (bound + 1e-300)).max()
    return bool(r <= 1.0), float(r)


def check_forward(cfg, inp, ref, out, tol):
    """out: x0 [rows, H] in the encoding, x0_bf16 or None, pre [rows, H], mean [rows], rstd [rows] (f32) with rows >= n_rows, every
    buffer pre-filled with NaN.  tol: emb_tolerances(...)[0]."""
    n, H, enc = ref["n_rows"], cfg["H"], cfg["dt"]
    info = dict(cfg, branches=emb_branches(cfg))
    x0, pre, mean, rstd = out["x0"].view(-1, H), out["pre"].view(-1, H), out["mean"], out["rstd"]
    for name in ("x0", "x0_bf16", "pre", "mean", "rstd"):        # packed rows at or past n_rows are never written
        if out.get(name) is not None:
            flat = out[name].reshape(-1)
            per = H if name in ("x0", "x0_bf16", "pre") else 1
            assert bool(torch.isnan(flat[n * per:].float()).all()), (info, name, "rows past n_rows were written")
            assert bool(torch.isfinite(flat[:n * per].float()).all()), (info, name, "non-finite output")
    # pre: the kernel only adds, in the reference's order
    assert same_bits(pre[:n], ref["pre_f32"]), (info, "pre differs from (e + p) + t in f32",
                                                  int((_bits(pre[:n]) != _bits(ref["pre_f32"])).any(dim=1).sum()), "rows")
    xmax = ref["pre"].abs().amax(dim=1)
    e_mean = float(((mean[:n].double() - ref["mean"]).abs() / (EMB_MEAN_TOL * xmax + 1e-300)).max())
    e_rstd = float(((rstd[:n].double() - ref["rstd"]).abs() / (EMB_RSTD_TOL * ref["rstd"])).max())
    print(f"emb {cfg['seed']} fwd tol {tol:.3e}: mean error / bound {e_mean:.3f}, rstd error / bound {e_rstd:.3f}")
    assert e_mean <= 1.0 and e_rstd <= 1.0, (info, e_mean, e_rstd)
    keep, scale, y = ref["keep"], ref["scale"], ref["y"]
    for name, enc_ in (("x0", enc), ("x0_bf16", BF16)):
        if out.get(name) is None:
            continue
        got = out[name].view(-1, H)[:n]
        assert bool((got[~keep] == 0).all()), (info, name, "a dropped element is not zero")
        # the survivors, brought back to the scale of y: the row maximum of y stays the yardstick whatever the mask dropped
        got_y = torch.where(keep, got.double() / scale, y)
        if enc_ == F32:
            err = rowrel(got_y, y)
            print(f"    {name} f32 row-relative error {err:.3e}")
            assert err < tol, (info, name, err, tol)
        else:
            ok, worst = _within(got_y, y, out16_bound(y, enc_, tol))
            print(f"    {name} {enc_} error / bound {worst:.3f}")
            assert ok, (info, name, worst)


def emb_bwd_bounds(cfg, inp, ref):
    """Element-wise bound of each f32 accumulator after the backward, for ANY order of the atomic adds:
        got = prev + unscale * sum of terms, so |got - prev - unscale * sum| <= sum_bound(rows + 8, |prev| + unscale * sum|terms|)
                                                                                 + unscale * sum of the terms' own f32 errors.
    The previous value is one of the summed terms (every atomic add rounds relative to the running total, which holds it); + 8 covers
    the per-block partial sums of dgamma / dbeta / dTy / the hot row.  The terms' own errors are those of the LayerNorm backward fed
    with f32 statistics (rowops_cases.ln_term_errors: "cs" for a row of dpre, "dg" for dy * xhat; the two f32 additions that made pre
    are two more roundings of the same size as the four counted for xhat there, inside the doubling LN_XHAT_ROUNDINGS carries), plus,
    where the incoming gradient goes through dropout, the rounding of the scale 65536 / (65536 - thr) and of the product with it.
    Terms and contributor counts come from the fp64 reference.  -> name -> (want fp64, bound fp64, contributor count per row)"""
    us = 1.0 if cfg["unscale"] is None else float(np.float32(cfg["unscale"]))
    d, dpre = ref["d"], ref["dpre"]
    terr = ln_term_errors(ref["pre"], d, ref, dpre, None)
    drop_err = 2.0 * U32 * d.abs() if (cfg["p_drop"] > 0 or cfg["p_drop_img"] > 0) else torch.zeros_like(d)
    dev = dpre.device
    out = {}
    for name, (idx, mask) in emb_scatter_plan(cfg, ref).items():
        prev = inp["prev"][name].to(dev).double()
        rows = prev.shape[0]
        cnt = torch.bincount(idx[mask], minlength=rows).double()
        mag = torch.zeros_like(prev).index_add_(0, idx[mask], dpre[mask].abs())
        err = torch.zeros_like(prev).index_add_(0, idx[mask], terr["cs"][mask])
        out[name] = (us * ref[name], sum_bound(cnt[:, None] + 8, prev.abs() + us * mag) + us * err, cnt)
    n = float(ref["n_rows"])
    for name, terms, err in (("dg", d * ref["xhat"], terr["dg"] + drop_err * ref["xhat"].abs()), ("db", d, drop_err)):
        prev = inp["prev"][name].to(dev).double()
        out[name] = (us * ref[name], sum_bound(n + 8, prev.abs() + us * terms.abs().sum(0)) + us * err.sum(0), None)
    return out


def check_backward(cfg, inp, ref, out, tol):
    """out: dE [V, H], dP [maxpos, H], dTy [2, H], dg [H], db [H] (f32, holding inp["prev"] before the call) and dimg [B * N, H] in the
    encoding, pre-filled with NaN, or None when N = 0.  tol: emb_tolerances(...)[1]."""
    H, V, N, pad, enc = cfg["H"], cfg["V"], cfg["N"], cfg["pad"], cfg["dt"]
    info = dict(cfg, branches=emb_branches(cfg))
    dev = ref["pre"].device
    bounds = emb_bwd_bounds(cfg, inp, ref)
    print(f"emb {cfg['seed']} bwd tol {tol:.3e}")
    for name in ACC:
        want, bound, cnt = bounds[name]
        prev = inp["prev"][name].to(dev)
        got = out[name].to(dev)
        assert bool(torch.isfinite(got).all()), (info, name)
        delta = got.double() - prev.double()
        ok, worst = _within(delta, want, bound)
        print(f"    {name} error / bound {worst:.3f}")
        assert ok, (info, name, worst, int(((delta - want).abs() > bound).any(dim=-1).sum()), "rows or columns outside")
        if name in ("dE", "dP"):                      # a row nothing maps to is not touched at all
            idle = cnt == 0
            assert same_bits(got[idle], prev[idle]), (info, name, "a row without a contributor changed")
    dE, prevE = out["dE"].to(dev), inp["prev"]["dE"].to(dev)
    text_tok = ref["tok"][~ref["is_img"]]
    if 0 <= pad < V:
        assert same_bits(dE[pad], prevE[pad]), (info, "the pad row received a look-up gradient")
    elif bool((text_tok == 0).any()):
        assert not same_bits(dE[0], prevE[0]), (info, "pad id -1: row 0 is an ordinary row and must receive its gradient")
    if EMB_HOT_TOKEN < V and pad != EMB_HOT_TOKEN and bool((text_tok == EMB_HOT_TOKEN).any()):
        want, bound, _ = bounds["dE"]
        delta = dE[EMB_HOT_TOKEN].double() - prevE[EMB_HOT_TOKEN].double()
        assert bool((delta != 0).any()) and _within(delta, want[EMB_HOT_TOKEN], bound[EMB_HOT_TOKEN])[0], (info, "hot row")
    if N == 0:
        assert out.get("dimg") is None
        return
    dimg = out["dimg"].to(dev).view(-1, H)
    img = ref["is_img"]
    region = (ref["b"] * N + ref["reg"])[img]
    written = torch.zeros(dimg.shape[0], dtype=torch.bool, device=dev)
    written[region] = True
    assert bool(torch.isnan(dimg[~written].float()).all()), (info, "dimg: a region outside the packed rows was written")
    if bool(img.any()):
        got, want = dimg[region], ref["dpre"][img]
        assert bool(torch.isfinite(got.float()).all()), (info, "dimg")
        if enc == F32:
            err = rowrel(got, want)
            print(f"    dimg f32 row-relative error {err:.3e}")
            assert err < tol, (info, "dimg", err, tol)
        else:
            ok, worst = _within(got, want, out16_bound(want, enc, tol))
            print(f"    dimg {enc} error / bound {worst:.3f}")
            assert ok, (info, "dimg", worst)


# =====================================================================================================================
# a plain f32 implementation (CPU): what the bounds above must let pass without any kernel
# =====================================================================================================================
def emb_plain_f32(cfg, inp, ref):
    """Forward and backward in f32 torch on the CPU, the LayerNorm written out by hand, tables updated with index_add_: the outputs in
    the layout check_forward / check_backward take.  The backward is fed as the sweep feeds the kernel: pre from the f32 expression,
    mean and rstd from the fp64 reference rounded to f32."""
    H, N, n, eps, dt = cfg["H"], cfg["N"], ref["n_rows"], cfg["eps"], DT[cfg["dt"]]
    rows = cfg["B"] * emb_L(cfg)
    pre = ref["pre_f32"].cpu()
    gamma, beta = inp["gamma"].float(), inp["beta"].float()
    keep, scale = ref["keep"].cpu(), ref["scale"].cpu().float()
    mu = pre.mean(dim=1, keepdim=True)
    rs = 1.0 / torch.sqrt(((pre - mu) ** 2).mean(dim=1, keepdim=True) + eps)
    y = ((pre - mu) * rs * gamma + beta) * keep * scale

    def padded(t, dtype):
        buf = torch.full((rows,) + tuple(t.shape[1:]), float("nan"), dtype=dtype)
        buf[:n] = t.to(dtype)
        return buf
    fwd = dict(x0=padded(y, dt), x0_bf16=padded(y, torch.bfloat16) if cfg["x0_bf16"] else None, pre=padded(pre, torch.float32),
               mean=padded(mu[:, 0], torch.float32), rstd=padded(rs[:, 0], torch.float32))
    us = 1.0 if cfg["unscale"] is None else float(np.float32(cfg["unscale"]))
    mean_r, rstd_r = ref["mean"].cpu().float()[:, None], ref["rstd"].cpu().float()[:, None]
    d = inp["dx0"].float() * keep * scale
    xhat = (pre - mean_r) * rstd_r
    gd = gamma * d
    dpre = rstd_r * (gd - gd.mean(dim=1, keepdim=True) - xhat * (gd * xhat).mean(dim=1, keepdim=True))
    bwd = {k: v.clone() for k, v in inp["prev"].items()}
    for name, (idx, mask) in emb_scatter_plan(cfg, ref).items():
        bwd[name].index_add_(0, idx[mask].cpu(), us * dpre[mask.cpu()])
    bwd["dg"] += us * (d * xhat).sum(0)
    bwd["db"] += us * d.sum(0)
    bwd["dimg"] = None
    if N:
        bwd["dimg"] = torch.full((cfg["B"] * N, H), float("nan"), dtype=dt)
        img = ref["is_img"].cpu()
        bwd["dimg"][(ref["b"] * N + ref["reg"]).cpu()[img]] = dpre[img].to(dt)
    return fwd, bwd
