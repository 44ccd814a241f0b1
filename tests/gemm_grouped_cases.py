"""Cases, restated plan, fp64 references and element-wise bounds of the grouped weight-gradient sweep (mv_gemm_grouped_tn:
csrc/mv_gemm_group.h, gemm_pring_grouped_kernel of mv_gemm_ring.h, splitk_reduce_grouped_kernel of mv_gemm_ring_tn.hip).

Plain module: nothing here touches the GPU or the HIP library.  tests/test_gemm_grouped_sweep_gpu.py runs the cases;
tests/test_gemm_grouped_cases_cpu.py compares group_plan() with the library's own map, counts what every case reaches and shows that
the bounds let an honest f32 computation through and catch each planted defect.

* group_plan() restates the tail rule, the XCD remap, the 8-row raster, the problem search and the kchunk rule from the comments of
  mv_gemm_group.h; branches() names what a case reaches in the kernel, the reduction and the per-block walk (the vmcnt accounting
  depends on what the PREVIOUS unit of a block was);
* a case is a table of problems (No, Ko, rows): C[No, Ko] (+)= alpha * A[rows, No]^T . B[rows, Ko]; its tensors are made from
  cfg["seed"] alone, so a cfg printed by a failing assertion reproduces the case;
* operands are contraction-major [rows, ld] as gemm_cases.operand makes them for the TN layout (everything right of the logical
  columns NaN) with GUARD_ROWS NaN rows below, or, form "slice", the engine's dqkv form: the middle third of a buffer 3 * No wide
  whose other two thirds are NaN.  C sits in a NaN buffer (guards right of Ko and below No) under one of four placements;
* reference: fp64 a.T @ b of the rounded inputs, times the f32 alpha, plus C0; bound of every element: gemm_cases.epilogue_reference,
  exactly as gemm_reference bounds an f32 split-K output -- sum_bound with rows + slices terms on S = |a|.T @ |b| (slices: the slabs
  the reduction adds for that element's tile, 1 for an unsplit tile), plus the f32 roundings of alpha and of the accumulate add.
  No constant of its own.

No case needed a wider bound.  Measured on an MI355X, largest error / bound per family: raster 0.23, walk 0.25, tail 0.23, layer 0.22,
grid 0.23 -- all in cases with alpha and accumulate, where the half-ulp roundings of those two operations are a quarter of the
EPI_ROUNDINGS = 4 roundings the bound grants; the product alone stays near 0.01 of its sum_bound share.
"""
import math

import torch

from gemm_cases import DEFAULT_CUS, EPI_NONE, GUARD_ROWS, NAN, cdiv, epilogue_reference, place, within  # noqa: F401
from rowops_cases import BF16, DT, F16, up

# ---- constants of the plan (tests/test_gemm_grouped_cases_cpu.py reads the same numbers out of the .h text) ----------------------
MAX_SPLIT, TILE, BK = 8, 256, 64
FILL_NUM, FILL_DEN = 7, 10                   # a split is taken when it fills its rounds to 70 %
GM = 8                                       # row tiles per group of the raster
EPI_OPS = 28                                 # VMEM ops a wave is known to have issued after a full tile's / a slab's epilogue
XCDS = 8


# =====================================================================================================================
# the plan restated
# =====================================================================================================================
def tail_split(R, G):
    """smallest s <= MAX_SPLIT for which R * s units fill the rounds of G blocks they occupy to 70 %; 1 when none does"""
    for s in range(1, MAX_SPLIT + 1):
        if R > 0 and FILL_DEN * R * s >= FILL_NUM * cdiv(R * s, G) * G:
            return s
    return 1


def xcd_remap(u, n):
    """unit u runs on block u mod G, blocks b, b + 8, ... share an XCD: XCD x takes one contiguous run of [0, n), the first n mod 8
    runs one longer"""
    q, r = divmod(n, XCDS)
    x, i = u % XCDS, u // XCDS
    return sum(q + 1 if k < r else q for k in range(x)) + i


def raster(t, No, Ko):
    """tile t of one problem -> (m0, n0, row group, gm): groups of GM row tiles, inside a group row-fastest"""
    tm, tn = cdiv(No, TILE), cdiv(Ko, TILE)
    group, rem = divmod(t, GM * tn)
    gm = min(GM, tm - group * GM)
    return (group * GM + rem % gm) * TILE, (rem // gm) * TILE, group, gm


def tiles_of(shape):
    return cdiv(shape[0], TILE) * cdiv(shape[1], TILE)


def group_plan(shapes, G):
    """-> (header dict(units, direct, tail, split, kchunk [per problem], unit0 [per problem]),
           [(problem, m0, n0, kbeg, kend, slice, tile)] per launch unit)"""
    unit0, U = [], 0
    for s in shapes:
        unit0.append(U)
        U += tiles_of(s)
    rem = U % G
    split = tail_split(rem, G)
    tail = rem if split > 1 else 0
    direct = U - tail
    kchunk = [up(cdiv(rows, split), BK) for _, _, rows in shapes]
    hdr = dict(units=U, direct=direct, tail=tail, split=split, kchunk=kchunk, unit0=unit0, n_blocks=G)
    units = []
    for u in range(direct + tail * split):
        if u < direct:
            tile, sl = xcd_remap(u, direct), -1
        else:
            sl, t = divmod(xcd_remap(u - direct, tail * split), tail)
            tile = direct + t
        prob = max(i for i in range(len(shapes)) if unit0[i] <= tile)
        No, Ko, rows = shapes[prob]
        m0, n0, _, _ = raster(tile - unit0[prob], No, Ko)
        kbeg, kend = (0, rows) if sl < 0 else (min(sl * kchunk[prob], rows), min((sl + 1) * kchunk[prob], rows))
        units.append((prob, m0, n0, kbeg, kend, sl, tile))
    return hdr, units


def workspace_bytes(hdr):
    return hdr["tail"] * hdr["split"] * TILE * TILE * 4 if hdr["split"] > 1 else 0


# =====================================================================================================================
# cases
# =====================================================================================================================
CPLACE = ("tight", "pad4", "odd", "off1")


def c_place(name, Ko):
    """-> (ldc, offset of C's base in floats)"""
    if name == "tight":
        return Ko, 0
    if name == "pad4":
        return up(Ko, 4) + 4, 0
    if name == "odd":
        return (Ko + 1 if Ko % 2 == 0 else Ko + 2), 0
    return up(Ko, 4) + 4, 1                                         # off1: C & 15 != 0


def base(fam, seed, shapes, G, **kw):
    n = len(shapes)
    c = dict(fam=fam, seed=seed, dt=BF16, shapes=tuple(tuple(s) for s in shapes), G=G, pcus=(0,), alpha=None, accumulate=0,
             cplace=tuple(("tight", "pad4")[i % 2] for i in range(n)), aform=("plain",) * n, launches=1, single=False)
    c.update(kw)
    return c


def case_id(c):
    s = "%s-%d-%s-%dp-G%d" % (c["fam"], c["seed"], c["dt"], len(c["shapes"]), c["G"])
    if c["pcus"] != (0,):
        s += "-cus" + "_".join(str(p) for p in c["pcus"])
    if c["alpha"] is not None:
        s += "-alpha"
    if c["accumulate"]:
        s += "-acc"
    return s


def layout(c):
    """per problem: dict(No, Ko, rows, lda, a_col, ldb, ldc, c_off, vec_ok)"""
    out = []
    for i, ((No, Ko, rows), form, cp) in enumerate(zip(c["shapes"], c["aform"], c["cplace"])):
        lda, a_col = (3 * No, No) if form == "slice" else (up(No, 8) + (8 if i % 2 else 0), 0)
        ldb = up(Ko, 8) + (0 if i % 2 else 8)
        ldc, off = c_place(cp, Ko)
        out.append(dict(No=No, Ko=Ko, rows=rows, lda=lda, a_col=a_col, ldb=ldb, ldc=ldc, c_off=off, vec_ok=ldc % 4 == 0 and off % 4 == 0))
    return out


def launch_blocks(c, pcus, n_cu=DEFAULT_CUS):
    """grid of the persistent launch: the plan's G, the CUs the knob leaves, never more blocks than units"""
    hdr, units = group_plan(c["shapes"], c["G"])
    return min(len(units), c["G"], pcus if 0 < pcus < n_cu else n_cu)


RASTER = ((2248, 260, 72), (3072, 768, 136), (768, 3072, 136), (2304, 768, 200), (520, 515, 333))
RASTER_G = (1, 5, 11, 13, 100, 256)
RASTER_PLANS = ((126, 0, 1), (125, 1, 4), (121, 5, 2), (117, 9, 4), (100, 26, 3), (0, 126, 2))
WALK = ((256, 256, 64), (200, 136, 333), (257, 261, 129), (256, 512, 40), (130, 70, 1), (512, 256, 448), (256, 256, 128))
WALK_ORDERS = ((0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (4, 0, 5, 3, 1, 6, 2))
WALK_G = (1, 2, 3, 5)                       # 12 tiles: unsplit on 1, 2 and 3 blocks; on 5 blocks two tiles are cut in halves
TAIL = ((512, 256, 448), (256, 256, 64), (200, 136, 333), (257, 261, 129), (130, 67, 100))
TAIL_G = (2, 4, 6, 7, 8, 16)
TAIL_PLANS = ((8, 1, 2), (8, 1, 3), (6, 3, 2), (7, 2, 3), (8, 1, 6), (0, 9, 3))
SPLIT8 = ((200, 136, 333), (250, 130, 129), (130, 67, 100), (256, 256, 448))      # one tile each on 11 blocks: cut 8 ways
LAYER = ((768, 3072, 136), (3072, 768, 136), (768, 768, 136), (2304, 768, 136))
LAYER_PLANS = ((1, 256, (0, 108, 2)), (2, 256, (216, 0, 1)), (2, 100, (200, 16, 5)))
ALPHA = 1.0 / 1024.0


def raster_cases():
    cases = []
    for d, dt in enumerate((BF16, F16)):
        for i, s in enumerate(RASTER):
            n = len(cases)
            cases.append(base("raster", 10 + i, (s,), tiles_of(s), dt=dt, single=True, alpha=ALPHA if (n % 2) else None, accumulate=(n // 2) % 2,
                              cplace=(CPLACE[(i + d) % 4] if s[1] % 4 else ("tight", "pad4")[(i + d) % 2],)))
        for j, G in enumerate(RASTER_G):
            n = len(cases)
            cases.append(base("raster", 20, RASTER, G, dt=dt, alpha=ALPHA if (n % 2) else None, accumulate=(n // 2) % 2,
                              cplace=("pad4", "tight", "pad4", "tight", CPLACE[(j + d) % 4])))
    return cases


def walk_cases():
    cases = []
    for o, order in enumerate(WALK_ORDERS):
        for g, G in enumerate(WALK_G):
            n = len(cases)
            shapes = tuple(WALK[k] for k in order)
            cp = tuple(CPLACE[(k + n) % 4] if WALK[k][1] % 4 else ("tight", "pad4")[k % 2] for k in order)
            cases.append(base("walk", 30 + o, shapes, G, dt=(BF16, F16)[n % 2], launches=2, accumulate=(n // 2) % 2,
                              alpha=ALPHA if (n // 3) % 2 else None, cplace=cp))
    return cases


def tail_cases():
    cases = []
    for G in TAIL_G:
        for al in (None, ALPHA):
            for acc in (0, 1):
                for p in range(4):
                    n = len(cases)
                    cp = ("tight", "pad4", "pad4", CPLACE[p], CPLACE[(p + 1 + n // 4) % 4])
                    cases.append(base("tail", 40, TAIL, G, dt=(BF16, F16)[(n // 4 + p) % 2], alpha=al, accumulate=acc, cplace=cp))
    for i, s in enumerate(SPLIT8):                  # MV_GROUP_MAX_SPLIT itself: one tile on 11 blocks
        n = len(cases)
        cases.append(base("tail", 50 + i, (s,), 11, dt=(BF16, F16)[i % 2], alpha=ALPHA if i % 2 else None, accumulate=(i // 2) % 2,
                          cplace=(CPLACE[i % 4] if s[1] % 4 else "tight",)))
    return cases


def layer_cases():
    cases = []
    for layers, G, _ in LAYER_PLANS:
        for dt in (BF16, F16):
            n = len(cases)
            cases.append(base("layer", 60 + layers, LAYER * layers, G, dt=dt, alpha=ALPHA, accumulate=n % 2,
                              aform=("plain", "plain", "slice", "plain") * layers, cplace=("tight", "tight", "tight", "tight") * layers))
    return cases


def grid_cases():
    cases = []
    for G, pcus in ((16, (0, 3)), (3, (0, 2))):     # planned for 16, launched on 16 and on 3 blocks; planned for 3, launched on 3 and on 2
        for acc in (0, 1):
            for dt in (BF16, F16):
                n = len(cases)
                cases.append(base("grid", 40, TAIL, G, dt=dt, pcus=pcus, accumulate=acc, alpha=ALPHA if n % 2 == 0 else None,
                                  cplace=("tight", "pad4", "pad4", CPLACE[n % 4], CPLACE[(n + 1) % 4])))
    return cases


FAMILIES = {"raster": raster_cases, "walk": walk_cases, "tail": tail_cases, "layer": layer_cases, "grid": grid_cases}


def all_cases():
    return [c for gen in FAMILIES.values() for c in gen()]


# =====================================================================================================================
# what a case reaches
# =====================================================================================================================
def unit_state(c, lay, hdr, unit):
    """what the kernel does with one launch unit: dict(kind direct | slice, full, nst, epi, problem)"""
    prob, m0, n0, kbeg, kend, sl, tile = unit
    p = lay[prob]
    nst = max(1, cdiv(kend - kbeg, BK))
    if sl >= 0:
        return dict(kind="slice", full=True, nst=nst, problem=prob, epi="partial_store", empty=kend == kbeg,
                    short=0 < kend - kbeg < hdr["kchunk"][prob])
    whole_cols = n0 + TILE <= p["Ko"]
    full = m0 + TILE <= p["No"] and whole_cols and p["Ko"] % 4 == 0 and p["vec_ok"]
    if not p["vec_ok"]:
        epi = "epi_all_slow_ldc" if p["ldc"] % 4 else "epi_all_slow_base"
    elif whole_cols:
        epi = "epi_all_fast"
    else:
        epi = "epi_mixed_N%4" if p["Ko"] % 4 else "epi_fast+past_N"
    return dict(kind="direct", full=full, nst=nst, problem=prob, epi=epi, empty=False, short=False)


def branches(c, n_cu=DEFAULT_CUS):
    hdr, units = group_plan(c["shapes"], c["G"])
    lay = layout(c)
    b = set()
    states = [unit_state(c, lay, hdr, u) for u in units]
    for (prob, m0, n0, kbeg, kend, sl, tile), st in zip(units, states):
        No, Ko, rows = c["shapes"][prob]
        _, _, group, gm = raster(tile - hdr["unit0"][prob], No, Ko)
        b.add("gm=%d" % gm)
        if n0 > 0:
            b.add("n0>0")
        if group > 0:
            b.add("row_group>=1")
        if st["kind"] == "direct":
            b.add(st["epi"])
            b.add("full=%d" % st["full"])
        else:
            b.add("slice_empty" if st["empty"] else "slice_nonempty")
            if st["short"]:
                b.add("slice_short")
    # the reduction: one block column per tail tile
    tail_probs = set()
    for tile in range(hdr["direct"], hdr["units"]):
        prob = max(i for i in range(len(lay)) if hdr["unit0"][i] <= tile)
        tail_probs.add(prob)
        p = lay[prob]
        m0, n0, _, _ = raster(tile - hdr["unit0"][prob], p["No"], p["Ko"])
        body = "reduce_vec" if (p["vec_ok"] and p["Ko"] % 4 == 0) else "reduce_scalar"
        b.add(body)
        if c["alpha"] is not None:
            b.add(body + "+alpha")
        if c["accumulate"]:
            b.add(body + "+accumulate")
        if m0 + TILE > p["No"]:
            b.add("reduce_skip_m")
        if n0 + TILE - 4 >= p["Ko"]:
            b.add("reduce_skip_n")
        if cdiv(p["rows"], hdr["kchunk"][prob]) < hdr["split"]:
            b.add("reduce_nsl<split")
    # the walk of every block, for every grid the case launches
    for pcus in c["pcus"]:
        grid = launch_blocks(c, pcus, n_cu)
        if 0 < pcus < c["G"]:
            b.add("plan_blocks>launch_blocks")
        for blk in range(grid):
            mine = list(range(blk, len(units), grid))
            if len(mine) >= 3:
                b.add("walk>=3_units")
            for u0, u1 in zip(mine, mine[1:]):
                prev, cur = states[u0], states[u1]
                was = "slice" if prev["kind"] == "slice" else ("full" if prev["full"] else "ragged")
                b.add("after_%s->%s" % (was, "nst=1" if cur["nst"] == 1 else "nst>1"))
                if prev["kind"] == "direct" and cur["kind"] == "slice":
                    b.add("direct->slice")
                p0, p1 = lay[prev["problem"]], lay[cur["problem"]]
                if prev["problem"] != cur["problem"] and (p0["lda"], p0["ldb"], p0["rows"]) != (p1["lda"], p1["ldb"], p1["rows"]):
                    b.add("problem_boundary")
    # the shape of the plan
    b.add("split=%s" % ("5|6" if hdr["split"] in (5, 6) else hdr["split"]))
    if hdr["direct"] == 0:
        b.add("direct=0")
    if hdr["tail"] == 0:
        b.add("tail=0")
    elif len(tail_probs) == 1:
        b.add("tail_in_one_problem")
    elif len({hdr["kchunk"][p] for p in tail_probs}) > 1:
        b.add("tail_spans_kchunks")
    else:
        b.add("tail_spans_problems")
    for form in c["aform"]:
        b.add("A_" + form)
    b.add("operands_" + c["dt"])
    return sorted(b)


def census(fam=None):
    count = {}
    for c in (FAMILIES[fam]() if fam else all_cases()):
        for name in branches(c):
            count[name] = count.get(name, 0) + 1
    return count


# =====================================================================================================================
# inputs
# =====================================================================================================================
_OPERANDS = {}


def _operands(c):
    """logical a [No, rows], b [Ko, rows] of every problem in the operand encoding (shared by the cases of one seed)"""
    key = (c["seed"], c["dt"], c["shapes"])
    if key not in _OPERANDS:
        out = []
        for i, (No, Ko, rows) in enumerate(c["shapes"]):
            g = torch.Generator().manual_seed(c["seed"] * 7919 + 13 + 101 * i)
            a = torch.randn((No, rows), generator=g)
            b = torch.randn((Ko, rows), generator=g) / math.sqrt(rows)
            out.append((a.to(DT[c["dt"]]), b.to(DT[c["dt"]])))
        _OPERANDS[key] = out
    return _OPERANDS[key]


def group_inputs(c):
    """CPU tensors of a case, per problem: a, b logical; A, B storage windows [rows + GUARD_ROWS, ld] (A: the slice the kernel is given
    starts at column a_col); C0 logical [No, Ko] f32 or None; the layout() entries"""
    out = []
    for i, ((a, b), p) in enumerate(zip(_operands(c), layout(c))):
        No, Ko, rows = p["No"], p["Ko"], p["rows"]
        _, A = place(torch.full((rows, 0), NAN, dtype=a.dtype), p["lda"], 0, GUARD_ROWS)
        A[:rows, p["a_col"]:p["a_col"] + No] = a.t()
        _, B = place(b.t().contiguous(), p["ldb"], 0, GUARD_ROWS)
        C0 = None
        if c["accumulate"]:
            g = torch.Generator().manual_seed(c["seed"] * 7919 + 17 + 101 * i)
            C0 = torch.randn((No, Ko), generator=g)
        out.append(dict(p, a=a, b=b, A=A, B=B, C0=C0))
    return out


def c_buffer(p):
    """C of one problem in its poisoned buffer -> (flat, window [No + GUARD_ROWS, ldc])"""
    x = p["C0"] if p["C0"] is not None else torch.full((p["No"], p["Ko"]), NAN)
    return place(x, p["ldc"], p["c_off"], GUARD_ROWS)


# =====================================================================================================================
# reference and bound
# =====================================================================================================================
_PRODUCTS = {}


def _products(c, device="cpu"):
    key = (c["seed"], c["dt"], c["shapes"])
    if key not in _PRODUCTS:
        out = []
        for a, b in _operands(c):
            a64, b64 = a.to(device).double(), b.to(device).double()
            out.append(((a64 @ b64.t()).cpu(), (a64.abs() @ b64.abs().t()).cpu()))
        _PRODUCTS[key] = out
    return _PRODUCTS[key]


def slices_of(c, hdr=None):
    """per problem: [No, Ko] float64, the slabs the reduction adds for each element's tile (1: an unsplit tile)"""
    hdr = hdr or group_plan(c["shapes"], c["G"])[0]
    out = []
    for i, (No, Ko, rows) in enumerate(c["shapes"]):
        s = torch.ones((No, Ko), dtype=torch.float64)
        for t in range(tiles_of((No, Ko))):
            if hdr["unit0"][i] + t >= hdr["direct"]:
                m0, n0, _, _ = raster(t, No, Ko)
                s[m0:m0 + TILE, n0:n0 + TILE] = cdiv(rows, hdr["kchunk"][i])
        out.append(s)
    return out


def group_reference(c, t, device="cpu"):
    """-> [(ref, bound)] per problem, float64 [No, Ko]"""
    cfg = dict(epi=EPI_NONE, alpha=c["alpha"], p_drop=0.0)
    out = []
    for (y, S), sl, p in zip(_products(c, device), slices_of(c), t):
        C0 = p["C0"].double() if p["C0"] is not None else None
        out.append(epilogue_reference(cfg, y, S, sl, p["rows"], None, None, C0)["C"])
    return out


# =====================================================================================================================
# the honest f32 computation of the plan and the planted defects (CPU)
# =====================================================================================================================
DEFECTS = ("alpha_scalar", "acc_tail", "n0_dropped", "gm_last_group", "slice_stage", "stale_empty", "ldc_next")


def defect_applies(defect, c):
    hdr, units = group_plan(c["shapes"], c["G"])
    lay = layout(c)
    tail_probs = {u[0] for u in units if u[5] >= 0}
    if defect == "alpha_scalar":
        return c["alpha"] is not None and any(not (lay[p]["vec_ok"] and lay[p]["Ko"] % 4 == 0) for p in tail_probs)
    if defect == "acc_tail":
        return bool(c["accumulate"]) and hdr["tail"] > 0
    if defect == "n0_dropped":
        return any(Ko > TILE for _, Ko, _ in c["shapes"])
    if defect == "gm_last_group":
        return any(cdiv(No, TILE) % GM and cdiv(Ko, TILE) > 1 for No, Ko, _ in c["shapes"])
    if defect == "slice_stage":
        return hdr["tail"] > 0
    if defect == "stale_empty":
        return any(u[5] >= 0 and u[3] == u[4] for u in units)
    if defect == "ldc_next":
        return any(lay[i]["ldc"] != lay[i + 1]["ldc"] for i in range(len(lay) - 1))
    raise KeyError(defect)


def _store(flat, off, ld, m0, n0, block, accumulate):
    """block written at rows m0.., columns n0.. of a matrix of leading dimension ld at flat[off:] (what falls outside the buffer is lost)"""
    r, k = block.shape
    idx = off + (m0 + torch.arange(r))[:, None] * ld + (n0 + torch.arange(k))[None, :]
    ok = idx < flat.numel()
    flat[idx[ok]] = (flat[idx[ok]] + block[ok]) if accumulate else block[ok]


def honest_group(c, t, defect=None):
    """the launch in plain f32 torch: unsplit tiles in one product, tail tiles as per-slice partial products summed in slab order,
    then alpha, then + C.  -> [window [No, Ko] f32] per problem"""
    hdr, _ = group_plan(c["shapes"], c["G"])
    al = torch.tensor(c["alpha"] if c["alpha"] is not None else 1.0, dtype=torch.float32)
    out = []
    for i, p in enumerate(t):
        No, Ko, rows, kc = p["No"], p["Ko"], p["rows"], hdr["kchunk"][i]
        a, b = p["a"].float(), p["b"].float()
        flat, win = c_buffer(p)
        tm, tn = cdiv(No, TILE), cdiv(Ko, TILE)
        for tl in range(tm * tn):
            m0, n0, group, gm = raster(tl, No, Ko)
            if defect == "gm_last_group" and gm < GM:
                rem = tl - group * GM * tn
                m0, n0 = (group * GM + rem % GM) * TILE, (rem // GM) * TILE
            if m0 >= No or n0 >= Ko:
                continue
            ta, tb = a[m0:m0 + TILE], b[n0:n0 + TILE]
            in_tail = hdr["unit0"][i] + tl >= hdr["direct"]
            scalar_body = not (p["vec_ok"] and Ko % 4 == 0)
            if not in_tail:
                y = ta @ tb.t()
            else:
                y = torch.zeros((ta.shape[0], tb.shape[0]))
                for s in range(hdr["split"]):
                    lo, hi = min(s * kc, rows), min((s + 1) * kc, rows)
                    if defect == "slice_stage" and s == 0:
                        hi = max(hi - BK, lo)
                    if hi > lo:
                        y = y + ta[:, lo:hi] @ tb[:, lo:hi].t()
                    elif defect == "stale_empty":
                        y = y + ta[:, :min(kc, rows)] @ tb[:, :min(kc, rows)].t()          # what slice 0 of an earlier launch left there
            if not (defect == "alpha_scalar" and in_tail and scalar_body):
                y = y * al
            ld = p["ldc"]
            if defect == "ldc_next" and i > 0 and tl == 0:
                ld = t[i - 1]["ldc"]
            if defect == "n0_dropped":
                n0 = 0
            _store(flat, p["c_off"], ld, m0, n0, y, bool(c["accumulate"]) and not (defect == "acc_tail" and in_tail))
        out.append(win[:No, :Ko].clone())
    return out
