"""Case generators, dispatch predicates, fp64 references and element-wise bounds of the GEMM sweep (csrc/mv_gemm.hip,
mv_gemm_common.h, mv_gemm_ring.h and the mv_gemm_ring_*.hip units; mv_gemm and mv_conv2d of include/medvill.h).

Plain module: nothing here touches the GPU or the HIP library.  tests/test_gemm_sweep_gpu.py runs the cases, and
tests/test_gemm_cases_cpu.py counts which route, reduce body and epilogue path every case takes, so that a retuned threshold
cannot quietly turn one test into a repeat of another.

* every generator returns a dict; the tensors of a case are made from cfg["seed"] alone, so a cfg printed by a failing
  assertion reproduces the case;
* plan() restates mv_gemm's dispatch (mv_gemm_plan.h: the route, the slab arithmetic, the variant table; and the epilogue conditions)
  with the CU count as a parameter and names everything a case reaches;
* the references are plain torch in float64 on the already-rounded inputs; none of them calls a kernel of this project;
* every output element gets its own bound from the arithmetic (no global maximum):
    the f32 product            2 (K + slabs) 2^-24 S[m, n],  S = |A| . |B|  (rowops_cases.sum_bound: any summation order),
    carried through the epilogue by its Lipschitz factor, plus EPI_ROUNDINGS f32 roundings of the epilogue's own operations
    relative to the magnitudes it adds or multiplies, plus the evaluation error of erf / exp / tanh where one is used,
    a 16-bit output            half an ulp of the encoding at |ref| + bound (f16: plus its subnormal quantum 2^-25).
  bf16 keeps 8 significant bits, so half an ulp is up to 2^-8 of the value; rowops_cases.U16 holds 2^-9 for bf16 (its
  out16_bound reaches 2^-8 through the row maximum), hence HALF_ULP_REL doubles that entry.

No clean kernel needed a wider product bound than sum_bound: the MFMA's internal accumulation order is one of the orders the
bound covers.  Measured on an MI355X, largest error / bound per family: 16-bit outputs 0.99 (the half ulp of the encoding, which is
attained), f32 outputs of the split-K reduce 0.001, colsum_part 0.007.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from rowops_cases import BF16, DT, F16, F16_SUBNORMAL_HALF_ULP, F32, U16, U32, dgelu64, dm_restated, dm_threshold, f32r, sum_bound, up

NAN = float("nan")
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_DGELU, EPI_RES, EPI_BIAS_TANH, EPI_BIAS_GELU_D, EPI_MUL, EPI_BIAS_RELU, \
    EPI_BIAS_RES_RELU = range(11)                                   # include/medvill.h
EPI_NAMES = ["NONE", "BIAS", "BIAS_GELU", "BIAS_RES", "DGELU", "RES", "BIAS_TANH", "BIAS_GELU_D", "MUL", "BIAS_RELU", "BIAS_RES_RELU"]
NEED_BIAS = (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_BIAS_TANH, EPI_BIAS_GELU_D, EPI_BIAS_RELU, EPI_BIAS_RES_RELU)
NEED_R = (EPI_BIAS_RES, EPI_DGELU, EPI_RES, EPI_MUL, EPI_BIAS_RES_RELU)
NEED_C2 = (EPI_BIAS_GELU, EPI_BIAS_GELU_D)
WIDE_E = (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU_D)                      # G2_WIDE_COND: 16-byte-store epilogues without R ...
WIDE_R = (EPI_MUL, EPI_RES, EPI_BIAS_RES)                           # ... and with a 16-bit R read in 16-byte pieces (r8_ok)
ACTIVATED = (EPI_BIAS_GELU, EPI_BIAS_TANH, EPI_BIAS_GELU_D, EPI_BIAS_RELU, EPI_BIAS_RES_RELU)
CONV_EPIS = (EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RES_RELU)
LAYOUTS = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1), "TNN": (1, 0)}          # y = x.W^T, dx = dy.W, dW = dy^T.x, A^T.B^T
LAYOUT_OF = {v: k for k, v in LAYOUTS.items()}
ESIZE = {F32: 4, BF16: 2, F16: 2}
HALF_ULP_REL = {BF16: 2.0 * U16[BF16], F16: U16[F16]}               # see the module docstring

# ---- constants of the dispatch (tests/test_gemm_cases_cpu.py reads the same numbers out of mv_gemm_plan.h and the .hip text) ----
GT_BM, GT_BN, GT_BK = 128, 128, 64           # the 128x128 kernel
G2_BM, G2_BK = 256, 32                       # the ring kernels: 256 rows, stages of 32 x KS
RING_320_ROWS = 320
BIG_MIN_M, BIG_MIN_N, BIG_MIN_T128, BIG_LONG_K = 256, 128, 128, 4096
WIDE_NT_MIN_N = 1024
ROUNDS_MIN_M, ROUNDS_MIN_N, ROUNDS_MIN_K = 2048, 256, 256
ROUND_COST = {"128": 75, "256": 85, "320": 112}        # whole-rounds rule: measured time of one round of each kernel
WIDE_COST = {"256": 8, "320": 10}                       # wide y = x.W^T rule: rounds x rows
SLOTS_128, SLOTS_128_SK, SLOTS_RING, SLOTS_RING_V128 = 512, 768, 256, 512
SK_MIN_K, SK_DEPTH, SK_CAP_128, SK_CAP_RING = 2048, 1024, 16, 32
VALU_TILE, VALU_BK = 64, 16
EPI_OPS = 28                                 # persistent kernel: VMEM ops counted after a full f32 / split-K tile's epilogue
STRIP = 64                                   # columns a wave owns in every MFMA kernel
DEFAULT_CUS = 256

# ---- tolerances of the functions the epilogues evaluate ------------------------------------------------------------------------
EPI_ROUNDINGS = 4                            # f32 roundings of an epilogue's own adds / multiplies (at most: + bias, dropout scale, + R, alpha)
DACT_TOL = 1e-5                              # gelu_erf' as mv_dact's tests bound it (tests/test_rowops_fuzz_gpu.py), absolute
# tanh and GELU itself: the epilogue measured on a K = 8 product whose f32 result is exact (z = (i / 16) (1 + j / 128), |z| < 16: 16
# significant bits), against the float64 function: tanh absolutely (|tanh| <= 1), GELU relative to 1 + |z| (its own size; that also
# holds the rounding of the f32 result).  The constant is 4 x the measured figure; tests/test_gemm_sweep_gpu.py measures both again
# and asserts that they stay below the constants.
TANH_MEASURED, GELU_MEASURED = 5.82e-8, 9.43e-8         # both the same on the 128x128 and on the ring kernel; constants 2.33e-7, 3.77e-7
TANH_TOL, GELU_TOL = 4 * TANH_MEASURED, 4 * GELU_MEASURED
LIP_GELU, LIP_DGELU = 1.13, 0.8              # sup |gelu'| = 1.129, sup |gelu''| = 2 phi(0) = 0.798


# =====================================================================================================================
# dispatch restated
# =====================================================================================================================
def cdiv(a, b):
    return (a + b - 1) // b


def gemm_route(ta, tb, M, N, K, splitk, f16, rows256=False, force=0, nj=0, rounds=1, n_cu=DEFAULT_CUS):
    """mv_gemm_plan.h: the route of mv_gemm_plan.  -> dict(big, variant, tiles, sk_auto, rule)"""
    tm2 = cdiv(M, 256)
    t256, t128 = tm2 * cdiv(N, 256), tm2 * cdiv(N, 128)
    wide_nt = (not ta) and (not tb) and N >= WIDE_NT_MIN_N
    big = force == 2 or (force == 0 and M >= BIG_MIN_M and N >= BIG_MIN_N and (K % 8 == 0 or (ta and tb)) and (wide_nt or bool(ta))
                         and (t128 >= BIG_MIN_T128 or (K >= BIG_LONG_K and splitk != 1)))
    r = dict(big=big, variant=0, sk_auto=1, tiles=0, rule="plain")
    rounds_on = rounds != 0 and force == 0 and nj == 0
    if rounds_on and not ta and not big and splitk <= 1 and M >= ROUNDS_MIN_M and N >= ROUNDS_MIN_N and N % 8 == 0 and K % 8 == 0 and K >= ROUNDS_MIN_K:
        tn = cdiv(N, 256)
        t320 = cdiv(M, RING_320_ROWS) * tn
        s128 = cdiv(M, GT_BM) * cdiv(N, GT_BN)
        c128 = cdiv(s128, 3 * n_cu) * ROUND_COST["128"]
        c256 = cdiv(t256, n_cu) * ROUND_COST["256"]
        c320 = (1 << 60) if rows256 else cdiv(t320, n_cu) * ROUND_COST["320"]
        if c256 < c128 and c256 <= c320:
            return dict(big=True, variant=14, sk_auto=1, tiles=t256, rule="rounds256")
        if c320 < c128 and c320 < c256:
            return dict(big=True, variant=10, sk_auto=1, tiles=t320, rule="rounds320")
        r["rule"] = "rounds_back_to_128"
    if rounds_on and big and not ta and not tb and not rows256 and splitk <= 1 and K % 8 == 0:
        tn = cdiv(N, 256)
        t320 = cdiv(M, RING_320_ROWS) * tn
        if cdiv(t320, n_cu) * WIDE_COST["320"] < cdiv(t256, n_cu) * WIDE_COST["256"]:
            return dict(big=True, variant=10, sk_auto=1, tiles=t320, rule="wide320")
        r["rule"] = "wide256"
    if big:
        v = nj if nj else (24 if ta else 14)
        if v == 10 and ta:
            v = 24
        if v == 2 and not (f16 and ta == tb):
            v = 24 if ta else 14
        v128 = v == 2
        r["variant"] = v
        r["tiles"] = t128 if v128 else (cdiv(M, RING_320_ROWS) * cdiv(N, 256) if v == 10 else t256)
        slots = SLOTS_RING_V128 if v128 else SLOTS_RING
        if v != 10 and r["tiles"] < slots and K >= SK_MIN_K:
            r["sk_auto"] = max(1, min(slots // r["tiles"], K // SK_DEPTH, SK_CAP_RING))
    else:
        r["tiles"] = cdiv(M, GT_BM) * cdiv(N, GT_BN)
        if r["tiles"] < SLOTS_128 and K >= SK_MIN_K:
            r["sk_auto"] = max(1, min(SLOTS_128_SK // r["tiles"], K // SK_DEPTH, SK_CAP_128))
    return r


def workspace_bytes(cfg, n_cu=DEFAULT_CUS):
    """mv_gemm_workspace_bytes under the case's knobs"""
    if cfg["dt"] == F32 or cfg["impl"] != 0:
        return 0
    r = gemm_route(cfg["ta"], cfg["tb"], cfg["M"], cfg["N"], cfg["K"], 0, cfg["dt"] == F16, False, cfg["force"], cfg["nj"], cfg["rounds"], n_cu)
    return r["sk_auto"] * cfg["M"] * cfg["N"] * 4 if r["sk_auto"] > 1 else 0


def ring_kernel(ta, tb, f16, v):
    """the kernel a routed variant runs (mv_gemm_plan.h: mv_plan_ring_kernel)"""
    if v == 4 and ta and tb:
        return "ring_tn4"
    if not ta and not tb:
        return ({2: "ring256x128", 10: "ring320"} if f16 else {24: "pring", 10: "ring320"}).get(v, "ring14")
    if not ta and tb:
        return ({10: "ring320"} if f16 else {24: "pring", 10: "ring320"}).get(v, "ring14")
    if ta and tb:
        return ({2: "ring256x128", 24: "pring"} if f16 else {24: "pring"}).get(v, "ring14")
    return {24: "pring"}.get(v, "ring14")


RING_TILE = {"ring14": (256, 256, 64), "pring": (256, 256, 64), "ring320": (320, 256, 64), "ring256x128": (256, 128, 32), "ring_tn4": (256, 256, 32)}
RING_STAGES = {"ring14": 2, "pring": 2, "ring320": 2, "ring256x128": 3, "ring_tn4": 4}


def ws_floats(cfg, n_cu=DEFAULT_CUS):
    """floats of workspace the case passes (None: no workspace)"""
    w = cfg["ws"]
    if w == "none":
        return None
    wish = workspace_bytes(cfg, n_cu) // 4
    if w == "exact":
        return wish
    if w == "short":
        return wish - 1
    return max(cfg["splitk"], 1, SK_CAP_RING) * cfg["M"] * cfg["N"]          # "ample"


def flags(cfg):
    """vec_ok / vec8_ok / r8_ok of mv_gemm (alignment is that of the element offsets: every base buffer is 256-byte aligned)"""
    epi, N = cfg["epi"], cfg["N"]
    ldc, ldr, ldc2, ldc3 = N + cfg["ldc_pad"], N + cfg["ldr_pad"], N + cfg["ldc2_pad"], N + cfg["ldc3_pad"]
    nb, nr, n2, c3 = epi in NEED_BIAS, epi in NEED_R, epi in NEED_C2, cfg["c3dt"] is not None
    csz = ESIZE[cfg["cdt"]]

    def al(off, esz, a):
        return (off * esz) % a == 0
    rsz = ESIZE[cfg["rdt"]] if nr else 4
    vec_ok = (ldc % 4 == 0 and al(cfg["c_off"], csz, 4 * csz) and (not c3 or (ldc3 % 4 == 0 and al(cfg["c3_off"], 2, 8)))
              and (not nb or al(cfg["bias_off"], 4, 16)) and (not nr or (ldr % 4 == 0 and al(cfg["r_off"], rsz, 4 * rsz)))
              and (not n2 or (ldc2 % 4 == 0 and al(cfg["c2_off"], csz, 4 * csz))))
    r8_ok = nr and cfg["rdt"] != F32 and ldr % 8 == 0 and al(cfg["r_off"], 2, 16)
    vec8_ok = (cfg["cdt"] != F32 and ldc % 8 == 0 and al(cfg["c_off"], 2, 16) and (not nb or al(cfg["bias_off"], 4, 16))
               and (not c3 or (ldc3 % 8 == 0 and al(cfg["c3_off"], 2, 16))) and (not n2 or (ldc2 % 8 == 0 and al(cfg["c2_off"], 2, 16))))
    return dict(vec_ok=vec_ok, r8_ok=r8_ok, vec8_ok=vec8_ok, ldc=ldc, ldr=ldr, ldc2=ldc2, ldc3=ldc3)


def plan(cfg, n_cu=DEFAULT_CUS):
    """mv_gemm restated: -> dict(kernel, variant, rule, slabs, kchunk, reduce, tile, branches)"""
    ta, tb, M, N, K = cfg["ta"], cfg["tb"], cfg["M"], cfg["N"], cfg["K"]
    f16 = cfg["dt"] == F16
    fl = flags(cfg)
    splitk = cfg["splitk"] if cfg["splitk"] >= 0 else 1
    mfma = cfg["dt"] != F32 and cfg["impl"] == 0
    if splitk == 0 and not mfma:
        splitk = 1
    wsf = ws_floats(cfg, n_cu)
    plain_f32 = cfg["epi"] == EPI_NONE and cfg["cdt"] == F32
    out = dict(variant=0, rule="plain")
    if mfma:
        r = gemm_route(ta, tb, M, N, K, splitk, f16, cfg["csum"], cfg["force"], cfg["nj"], cfg["rounds"], n_cu)
        out.update(variant=r["variant"], rule=r["rule"], tiles=r["tiles"], sk_auto=r["sk_auto"])
        if r["big"]:
            sk = splitk
            if splitk > 1 or splitk == 0:
                sk = r["sk_auto"]
                if splitk > 1 and sk > splitk:
                    sk = splitk
                if sk > 1 and wsf is not None:
                    fit = wsf // (M * N)
                    if sk > fit:
                        sk = max(fit, 1)
                if sk > 1 and (wsf is None or not plain_f32):
                    sk = 1
            kchunk = up(cdiv(K, sk), 64)
            out["kernel"] = ring_kernel(ta, tb, f16, r["variant"])
            out["tile"] = RING_TILE[out["kernel"]]
        else:
            if splitk == 0:
                splitk = 1
                if r["sk_auto"] > 1 and wsf is not None and plain_f32:
                    splitk = r["sk_auto"] if wsf >= r["sk_auto"] * M * N else 1
            kchunk = up(cdiv(K, splitk), GT_BK)
            out["kernel"] = "mfma128_2stage" if (cfg["nj"] == 32 and not f16) else "mfma128"
            out["tile"] = (GT_BM, GT_BN, GT_BK)
    else:
        kchunk = up(cdiv(K, splitk), VALU_BK)
        out["kernel"] = "valu"
        out["tile"] = (VALU_TILE, VALU_TILE, VALU_BK)
    slabs = cdiv(K, kchunk)
    out.update(kchunk=kchunk, slabs=slabs)
    # the reduce kernel's three bodies
    if slabs == 1:
        out["reduce"] = "reduce_none"
    elif N % 4:
        out["reduce"] = "reduce_scalar"
    elif fl["vec_ok"] and fl["ldc"] % 4 == 0:
        out["reduce"] = "reduce_fast4"
    else:
        out["reduce"] = "reduce_slow4"
    b = [out["kernel"], "layout_" + LAYOUT_OF[(ta, tb)], "operands_" + cfg["dt"], "slabs=%d" % slabs, out["reduce"], "epi_" + EPI_NAMES[cfg["epi"]],
         "C_" + cfg["cdt"]]
    if out["rule"] != "plain":
        b.append("route_" + out["rule"])
    if out["kernel"].startswith(("ring", "pring")):
        b.append("variant=%d" % out["variant"])
        nst = cdiv(min(kchunk, K), out["tile"][2])
        ring = RING_STAGES[out["kernel"]]
        b.append("stages<ring" if nst < ring else ("stages=ring" if nst == ring else "stages>ring"))
    if cfg["splitk"] > 1 and slabs != cfg["splitk"]:
        b.append("slabs_clamped")
    if cfg["epi"] in NEED_R:
        b.append("R_" + cfg["rdt"])
    if cfg["c3dt"]:
        b.append("C3_" + cfg["c3dt"])
    if cfg["accumulate"]:
        b.append("accumulate")
    if cfg["alpha"] is not None:
        b.append("alpha")
        if slabs > 1:
            b.append(out["reduce"] + "+alpha")
    if slabs > 1 and cfg["accumulate"]:
        b.append(out["reduce"] + "+accumulate")
    if cfg["p_drop"] > 0:
        b.append("dropout")
    if cfg["csum"]:
        b.append("csum")
    if K % out["tile"][2]:
        b.append("ragged_last_k_tile")
    if K % 8:
        b.append("K%8")
    if M % out["tile"][0]:
        b.append("ragged_last_row_tile")
    # the epilogue path of every 64-column strip (a wave's share of a tile in all MFMA kernels)
    for path in strip_paths(cfg, out, fl):
        b.append(path)
    if out["kernel"] == "pring":
        tm, tn = cdiv(M, 256), cdiv(N, 256)
        units = tm * tn * slabs
        blocks = min(units, cfg["pcus"] if 0 < cfg["pcus"] < n_cu else n_cu)
        full = [(i + 1) * 256 <= M and (j + 1) * 256 <= N and N % 4 == 0 and (slabs > 1 or fl["vec_ok"]) for i in range(tm) for j in range(tn)]
        waited = any(full) and (slabs > 1 or cfg["cdt"] == F32)
        b.append("pring_full_tiles" if all(full) else ("pring_full+ragged_tiles" if any(full) else "pring_ragged_tiles"))
        if units > blocks:                             # some block walks on to a second unit: the issue cursor crosses a unit boundary
            b.append("pring_multi_unit_walk")
            if waited:
                b.append("pring_epi_ops_wait")
        if units >= 3 * blocks:
            b.append("pring_walk>=3_units_per_block")
        out["units_per_block"] = units / blocks
    out["branches"] = b
    return out


def strip_paths(cfg, pl, fl):
    """names of the epilogue paths the case's column strips take (each once)"""
    N, epi = cfg["N"], cfg["epi"]
    if pl["slabs"] > 1:
        return ["partial_store" + ("_ragged" if N % 4 else "")]
    if pl["kernel"] == "valu":
        return ["slow"]
    wide_epi = (epi in WIDE_E or (epi in WIDE_R and fl["r8_ok"])) and fl["vec8_ok"] and cfg["cdt"] != F32 and not cfg["accumulate"]
    paths = set()
    for s in range(cdiv(N, STRIP)):
        whole = (s + 1) * STRIP <= N
        if wide_epi and whole:
            paths.add("wide16")
            if epi in WIDE_R:
                paths.add("wide16_R")
        elif not fl["vec_ok"]:
            paths.add("slow")
        else:
            paths.add("fast4")
            if not whole and N % 4:
                paths.add("slow")                      # the ragged last group of 4 columns
            if epi in NEED_R and pl["kernel"] != "mfma128" and pl["kernel"] != "mfma128_2stage":
                paths.add("fast4_R_ahead" if whole else "fast4_R_inline")       # HAS_R && __all(lane_fast || !col_on)
    if "wide16" in paths and len(paths - {"wide16", "wide16_R"}):
        paths.add("wide16+ragged_neighbour")
    return sorted(paths)


def slab_edges(cfg, n_cu=DEFAULT_CUS):
    """contraction indices that are the first or last 8 of a K slab"""
    pl = plan(cfg, n_cu)
    K, kc = cfg["K"], pl["kchunk"]
    idx = set()
    for s in range(pl["slabs"]):
        lo, hi = s * kc, min(K, (s + 1) * kc)
        idx.update(range(lo, min(lo + 8, hi)))
        idx.update(range(max(hi - 8, lo), hi))
    return sorted(idx)


# =====================================================================================================================
# case generators
# =====================================================================================================================
def base(fam, seed, **kw):
    c = dict(fam=fam, seed=seed, dt=BF16, ta=0, tb=0, M=1, N=4, K=8, force=0, nj=0, impl=0, rounds=1, pcus=0, epi=EPI_NONE, cdt=F32, rdt=None,
             c3dt=None, ldc_pad=0, ldr_pad=0, ldc2_pad=0, ldc3_pad=0, c_off=0, r_off=0, c2_off=0, c3_off=0, bias_off=0, a_pad=0, b_pad=0,
             p_drop=0.0, drop_key=0, splitk=1, ws="none", accumulate=0, alpha=None, csum=False, edge4=False, launches=1)
    c.update(kw)
    if c["epi"] in NEED_R and c["rdt"] is None:
        c["rdt"] = F32
    return c


def case_id(c):
    s = "%s-%d-%s%s-%dx%dx%d-%s-%s" % (c["fam"], c["seed"], c["dt"], LAYOUT_OF[(c["ta"], c["tb"])] if "ta" in c else "", c["M"], c["N"], c["K"],
                                      EPI_NAMES[c["epi"]], c["cdt"])
    if c.get("force") or c.get("nj"):
        s += "-f%dv%d" % (c["force"], c["nj"])
    if c.get("splitk", 1) != 1:
        s += "-sk%d" % c["splitk"]
    return s


SMALL_M, SMALL_N, SMALL_K = (1, 127, 128, 129, 300), (2, 4, 6, 64, 130, 192, 260), (8, 56, 64, 72, 128, 200)
SMALL_DL = [(BF16, "NT"), (BF16, "NN"), (BF16, "TN"), (BF16, "TNN"), (F16, "NT"), (F16, "NN"), (F16, "TN")]
SMALL_EPI = (EPI_NONE, EPI_BIAS, EPI_RES, EPI_MUL, EPI_BIAS_RES)      # (the activations: epi family; tiny outputs would let a ReLU hide a defect)
N_SMALL = 84


def out_draw(rs, epi, allow_c3=True):
    cdt = [F32, BF16, F16][rs.randint(3)]
    kw = dict(cdt=cdt)
    if epi in NEED_R:
        kw["rdt"] = [F32, BF16, F16][rs.randint(3)]
    if allow_c3 and rs.randint(3) == 0:
        kw["c3dt"] = [BF16, F16][rs.randint(2)]
    return kw


def small_case(seed):
    rs = np.random.RandomState(8000 + seed)
    dt, lay = SMALL_DL[seed % len(SMALL_DL)]
    ta, tb = LAYOUTS[lay]
    nj = (0, 32)[(seed // len(SMALL_DL)) % 2]
    M = int(SMALL_M[seed % len(SMALL_M)]) if seed < 2 * len(SMALL_M) else int(rs.choice(SMALL_M))
    N = int(SMALL_N[(seed // 2) % len(SMALL_N)]) if seed < 2 * len(SMALL_N) else int(rs.choice(SMALL_N))
    K = int(SMALL_K[(seed // 3) % len(SMALL_K)]) if seed < 3 * len(SMALL_K) else int(rs.choice(SMALL_K))
    epi = int(SMALL_EPI[rs.randint(len(SMALL_EPI))])
    return base("small", seed, dt=dt, ta=ta, tb=tb, M=M, N=N, K=K, force=1, nj=nj, epi=epi, edge4=seed % 3 == 0,
                a_pad=int(rs.choice([0, 8])), b_pad=int(rs.choice([0, 8])), **out_draw(rs, epi))


def small_cases():
    return [small_case(s) for s in range(N_SMALL)]


RING_NJ = (14, 24, 10, 2, 4)
# (nj, operand dtype, layout) where the launcher runs a kernel of its own for that variant
RING_COMBOS = ([(14, BF16, l) for l in ("NT", "NN", "TN", "TNN")] + [(14, F16, l) for l in ("NT", "NN", "TN")]
               + [(24, BF16, l) for l in ("NT", "NN", "TN", "TNN")] + [(24, F16, "TN")]
               + [(10, d, l) for d in (BF16, F16) for l in ("NT", "NN")] + [(2, F16, "NT"), (2, F16, "TN")] + [(4, BF16, "TN"), (4, F16, "TN")])
RING_M, RING_M320 = (255, 256, 257, 513), (319, 320, 321, 641)
RING_N = (128, 130, 256, 260, 320, 520)
RING_K64, RING_K32 = (32, 64, 72, 128, 192, 264), (32, 40, 64, 96, 128, 160)
RING_EPI = (EPI_NONE, EPI_NONE, EPI_BIAS, EPI_RES, EPI_MUL, EPI_BIAS_RES, EPI_BIAS_GELU_D)
N_RING = 4 * len(RING_COMBOS)


def ring_variant_differs(nj, dt, lay):
    """the predicate of the draw: this (variant, operand encoding, layout) reaches a launcher branch of its own"""
    ta, tb = LAYOUTS[lay]
    if lay == "TNN" and dt == F16:
        return False
    if nj == 14:
        return True
    v = gemm_route(ta, tb, 256, 256, 64, 1, dt == F16, False, 2, nj)["variant"]
    return v == nj and ring_kernel(ta, tb, dt == F16, v) != "ring14"


def ring_case(seed):
    rs = np.random.RandomState(8100 + seed)
    nj, dt, lay = RING_COMBOS[seed % len(RING_COMBOS)]
    ta, tb = LAYOUTS[lay]
    rnd = seed // len(RING_COMBOS)
    ms = RING_M + (RING_M320 if nj == 10 else ())
    M = int(ms[(seed + rnd) % len(ms)])
    N = int(RING_N[(seed // 2 + rnd) % len(RING_N)])
    ks = RING_K32 if nj in (2, 4) else RING_K64
    K = int(ks[(seed // 3 + rnd) % len(ks)])
    epi = int(RING_EPI[rs.randint(len(RING_EPI))])
    kw = out_draw(rs, epi)
    csum = False
    if nj == 14 and rnd % 2 == 1:                    # fused column sums: N % 256 == 0, the 16-byte-store epilogue
        N, csum = 256, True
        epi = int((EPI_NONE, EPI_BIAS, EPI_BIAS_GELU_D, EPI_MUL, EPI_RES)[seed % 5])
        kw = dict(cdt=[BF16, F16][seed % 2], rdt=[BF16, F16][(seed // 2) % 2] if epi in NEED_R else None)
    return base("ring", seed, dt=dt, ta=ta, tb=tb, M=M, N=N, K=K, force=2, nj=nj, epi=epi, edge4=seed % 3 == 0, csum=csum,
                a_pad=int(rs.choice([0, 8])), b_pad=int(rs.choice([0, 8])), **kw)


def ring_cases():
    return [ring_case(s) for s in range(N_RING)]


PRING_SHAPES, PRING_K, PRING_CUS = ((768, 520), (513, 768), (1024, 260)), (64, 200), (3, 5)
PRING_MODES = ("none", "accumulate", "bias_res_bf16", "splitk2")


def pring_cases():
    cases = []
    for i, (M, N) in enumerate(PRING_SHAPES):
        for j, K in enumerate(PRING_K):
            for m, mode in enumerate(PRING_MODES):
                nj = (24, 14)[(i + j + m) % 2] if mode != "splitk2" else 24
                lay = ("TN", "NT", "NN", "TNN")[(i + 2 * j + m) % 4]
                ta, tb = LAYOUTS[lay]
                kw = dict(dt=BF16, ta=ta, tb=tb, M=M, N=N, K=K, force=2, nj=nj, pcus=PRING_CUS[(i + j + m) % 2], launches=2, edge4=(i + m) % 3 == 0)
                if mode == "accumulate":
                    kw.update(accumulate=1)
                elif mode == "bias_res_bf16":
                    kw.update(epi=EPI_BIAS_RES, cdt=BF16, rdt=BF16)
                elif mode == "splitk2":
                    kw.update(splitk=2, ws="ample", K=K + SK_MIN_K)       # the ring kernels split only from K = 2048 on, into slabs at least 1024 deep
                cases.append(base("pring_walk", len(cases), **kw))
    return cases


VALU_MN, VALU_K = (1, 63, 64, 65, 130), (1, 15, 16, 17, 72)
N_VALU = 48


def valu_case(seed):
    rs = np.random.RandomState(8200 + seed)
    dt = (BF16, F16, F32)[seed % 3]
    ta, tb = LAYOUTS[("NT", "NN", "TN", "TNN")[(seed // 3) % 4]]
    M = int(VALU_MN[seed % 5])
    N = int(VALU_MN[(seed // 5) % 5]) if seed < 25 else int(rs.choice(VALU_MN))
    K = int(VALU_K[(seed // 2) % 5])
    sk = (1, 3)[(seed // 4) % 2]
    epi = EPI_NONE if sk > 1 else int(SMALL_EPI[rs.randint(len(SMALL_EPI))])
    kw = out_draw(rs, epi) if sk == 1 else dict(cdt=F32)
    return base("valu", seed, dt=dt, ta=ta, tb=tb, M=M, N=N, K=K, impl=1, epi=epi, splitk=sk, ws="ample" if sk > 1 else "none",
                accumulate=int(sk > 1 and seed % 2), alpha=0.25 if (sk > 1 and seed % 3 == 0) else None, edge4=seed % 3 == 1, **kw)


def valu_cases():
    return [valu_case(s) for s in range(N_VALU)]


# (M, N, K, layout, splitk, colsum_part, rounds knob, the route it must take at 256 CUs: rule, kernel, slabs)
AUTO_TABLE = [
    (4224, 3072, 256, "NN", 1, False, 1, ("rounds256", "ring14", 1)),
    (21761, 768, 256, "NT", 1, False, 1, ("rounds320", "ring320", 1)),
    (21761, 768, 256, "NN", 1, False, 1, ("rounds320", "ring320", 1)),
    (27201, 768, 256, "NT", 1, False, 1, ("rounds_back_to_128", "mfma128", 1)),
    (16385, 1024, 64, "NT", 1, False, 1, ("wide320", "ring320", 1)),
    (16384, 1024, 64, "NT", 1, False, 1, ("wide256", "ring14", 1)),
    (4096, 1024, 64, "NT", 1, False, 1, ("wide256", "ring14", 1)),
    (2048, 1024, 64, "NT", 1, False, 1, ("plain", "mfma128", 1)),
    (2048, 2048, 64, "TN", 1, False, 1, ("plain", "pring", 1)),
    (2048, 2048, 64, "TNN", 1, False, 1, ("plain", "pring", 1)),
    (256, 128, 4096, "TN", 0, False, 1, ("plain", "pring", 4)),
    (512, 256, 8192, "TN", 0, False, 1, ("plain", "pring", 8)),
    (256, 256, 2048, "TN", 0, False, 1, ("plain", "mfma128", 2)),
    (4352, 3072, 256, "NN", 1, True, 1, ("rounds256", "ring14", 1)),
    (4224, 3072, 256, "NN", 1, False, 0, ("plain", "mfma128", 1)),
    (21761, 768, 256, "NT", 1, False, 0, ("plain", "mfma128", 1)),
    # one more of each rule, so that every route name is reached three times
    (4224, 3072, 512, "NN", 1, False, 1, ("rounds256", "ring14", 1)),
    (21761, 768, 512, "NT", 1, False, 1, ("rounds320", "ring320", 1)),
    (27201, 768, 256, "NN", 1, False, 1, ("rounds_back_to_128", "mfma128", 1)),
    (27201, 768, 512, "NT", 1, False, 1, ("rounds_back_to_128", "mfma128", 1)),
    (16385, 1024, 128, "NT", 1, False, 1, ("wide320", "ring320", 1)),
    (16385, 2048, 64, "NT", 1, False, 1, ("wide320", "ring320", 1)),
    (16384, 1024, 128, "NT", 1, False, 1, ("wide256", "ring14", 1)),
]
AUTO_BIG_ROWS = 16000            # above this the GPU file computes the reference on the device


def auto_cases():
    cases = []
    for i, (M, N, K, lay, sk, csum, rounds, _) in enumerate(AUTO_TABLE):
        ta, tb = LAYOUTS[lay]
        dt = F16 if (i % 2 and lay != "TNN") else BF16
        kw = dict(dt=dt, ta=ta, tb=tb, M=M, N=N, K=K, rounds=rounds, splitk=sk, csum=csum, edge4=i % 3 == 0)
        if sk == 0:
            kw.update(ws="exact", cdt=F32, alpha=0.5 if i % 2 else None)
        else:
            kw.update(cdt=[BF16, F16][i % 2], epi=EPI_BIAS if not csum else EPI_BIAS_GELU_D)
        cases.append(base("auto", i, **kw))
    return cases


REDUCE_KERNELS = (("mfma128", dict(force=1)), ("ring14", dict(force=2, nj=14)), ("pring", dict(force=2, nj=24)), ("valu", dict(impl=1)))
# (N, ldc pad, C offset in floats): the body of splitk_reduce_kernel each takes
REDUCE_SHAPES = ((136, 0, 0, "reduce_fast4"), (200, 0, 0, "reduce_fast4"), (136, 1, 0, "reduce_slow4"), (136, 0, 1, "reduce_slow4"),
                 (130, 0, 0, "reduce_scalar"), (135, 0, 0, "reduce_scalar"), (137, 0, 0, "reduce_scalar"))
REDUCE_SLABS = (2, 4, 7, 0)
REDUCE_M, REDUCE_K = 200, 4100


def reduce_cases():
    cases = []
    for ki, (kname, knobs) in enumerate(REDUCE_KERNELS):
        for si, (N, pad, off, _) in enumerate(REDUCE_SHAPES):
            for acc in (0, 1):
                for al in (None, 0.25):
                    n = len(cases)
                    sk = REDUCE_SLABS[(ki + si + 2 * acc + (al is not None)) % 4]
                    lay = ("TN", "NT", "NN")[(si + ki) % 3]
                    ta, tb = LAYOUTS[lay]
                    dt = BF16 if (kname == "pring" and lay != "TN") else (BF16, F16)[(n // 2) % 2]      # f16: persistent form for dW only
                    cases.append(base("reduce", n, dt=dt, ta=ta, tb=tb, M=REDUCE_M, N=N, K=REDUCE_K, ldc_pad=pad, c_off=off,
                                      splitk=sk, ws="ample", accumulate=acc, alpha=al, edge4=n % 3 == 0, **knobs))
    return cases


def workspace_cases():
    cases = []
    for i, (M, N, K, force) in enumerate(((256, 128, 4096, 0), (512, 256, 8192, 0), (256, 256, 2048, 0), (200, 136, 4100, 1), (300, 260, 3072, 2))):
        for ws in ("exact", "short", "none"):
            cases.append(base("workspace", len(cases), dt=(BF16, F16)[i % 2], ta=1, tb=1, M=M, N=N, K=K, force=force, splitk=0, ws=ws,
                              accumulate=i % 2, alpha=0.25 if i % 3 == 0 else None, edge4=i % 2 == 0))
    return cases


EPI_SHAPES = ((300, 384, 72), (257, 320, 128), (130, 132, 64))
EPI_KERNELS = (dict(force=1), dict(force=1, nj=32), dict(force=2, nj=14), dict(force=2, nj=24), dict(force=2, nj=10))
EPI_LD = (0, 8, 4)


def epi_cases():
    cases = []
    for epi in range(11):
        for ki, knobs in enumerate(EPI_KERNELS):
            for rep in range(2):
                n = len(cases)
                rs = np.random.RandomState(8400 + n)
                M, N, K = EPI_SHAPES[(epi + ki + rep) % 3]
                lay = ("NT", "NN", "TN", "TNN")[(n // 3) % 4]
                if knobs.get("nj") == 10 and lay in ("TN", "TNN"):
                    lay = ("NT", "NN")[n % 2]
                dt = F16 if (n % 3 == 1 and lay != "TNN") else BF16
                ta, tb = LAYOUTS[lay]
                path = n % 4            # 0: everything aligned (the wide path where the epilogue has one) | 1: ld + 4 | 2: one base off | 3: drawn
                cdt = [BF16, F16, F32][(n // 2) % 3] if path else [BF16, F16][n % 2]
                kw = dict(cdt=cdt)
                if epi in NEED_R:
                    kw["rdt"] = [BF16, F16, F32][(n // 5) % 3] if path else [BF16, F16][(n // 2) % 2]
                if rep == 1 or n % 5 == 0:
                    kw["c3dt"] = [BF16, F16][(n // 7) % 2]
                lds = dict(ldc_pad=0, ldr_pad=0, ldc2_pad=0, ldc3_pad=0)
                if path == 0:
                    lds = {k: int(rs.choice([0, 8])) for k in lds}
                elif path == 1:
                    lds[("ldc_pad", "ldr_pad", "ldc2_pad", "ldc3_pad")[n % 4 if (n % 4 != 1 or epi in NEED_R) else 0]] = 4
                elif path == 3:
                    lds = {k: int(rs.choice(EPI_LD)) for k in lds}
                offs = dict(c_off=0, r_off=0, c2_off=0, c3_off=0, bias_off=0)
                if path == 2:
                    which = ["c_off"] + (["r_off"] if epi in NEED_R else []) + (["c2_off"] if epi in NEED_C2 else []) + \
                            (["c3_off"] if "c3dt" in kw else []) + (["bias_off"] if epi in NEED_BIAS else [])
                    offs[which[(n // 4) % len(which)]] = 1
                if epi == EPI_BIAS_RES and rep == 1:
                    kw.update(p_drop=0.1, drop_key=int(rs.randint(1, 2 ** 31)) * 65537 + 12345)
                cases.append(base("epi", n, dt=dt, ta=ta, tb=tb, M=M, N=N, K=K, epi=epi, edge4=n % 3 == 0, **knobs, **kw, **lds, **offs))
    return cases


# ---- convolution ----------------------------------------------------------------------------------------------------
CONV_C, CONV_O, CONV_K, CONV_S, CONV_P, CONV_B = (8, 16, 64), (4, 64, 132), (1, 3, 7), (1, 2), (0, 1, 3), (1, 3)
N_CONV = 48


def conv_case(seed):
    rs = np.random.RandomState(8500 + seed)
    C, O, k = int(CONV_C[seed % 3]), int(CONV_O[(seed // 3) % 3]), int(CONV_K[(seed // 9) % 3 if seed < 27 else rs.randint(3)])
    s, p, B = int(CONV_S[seed % 2]), int(CONV_P[(seed // 2) % 3]), int(CONV_B[(seed // 4) % 2])
    H = int(rs.randint(5, 14))
    W = int(rs.randint(5, 14))
    if W == H:
        W = H + 1 if H < 13 else H - 1
    if seed % 4 == 3:
        H, W, B, s = 13, 12, 3, 1                        # B x Ho x Wo well past 128 rows: image boundaries inside row tiles
    if H + 2 * p < k or W + 2 * p < k:
        p = 3
    epi = int(CONV_EPIS[(seed // 2) % 4])
    return dict(fam="conv", seed=seed, C=C, O=O, k=k, s=s, p=p, H=H, W=W, B=B, epi=epi, cdt=(F32, BF16)[(seed // 3) % 2],
                rdt=(F32, BF16)[(seed // 5) % 2] if epi == EPI_BIAS_RES_RELU else None, edge4=seed % 3 == 0)


def conv_cases():
    return [conv_case(s) for s in range(N_CONV)]


def conv_id(c):
    return "conv-%d-C%dO%dk%ds%dp%d-%dx%dx%d-%s-%s" % (c["seed"], c["C"], c["O"], c["k"], c["s"], c["p"], c["B"], c["H"], c["W"], EPI_NAMES[c["epi"]], c["cdt"])


def conv_dims(c):
    Ho = (c["H"] + 2 * c["p"] - c["k"]) // c["s"] + 1
    Wo = (c["W"] + 2 * c["p"] - c["k"]) // c["s"] + 1
    return Ho, Wo, c["B"] * Ho * Wo, c["k"] * c["k"] * c["C"]


def conv_branches(c):
    """tile classes of the implicit-GEMM staging (gemm_mfma_kernel<.., CONV = true>: 128-row x 64-deep tiles)"""
    Ho, Wo, M, K = conv_dims(c)
    k, s, p, H, W, C = c["k"], c["s"], c["p"], c["H"], c["W"], c["C"]
    m = np.arange(M)
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    names = set()
    for t0 in range(0, M, GT_BM):
        rows = slice(t0, min(t0 + GT_BM, M))
        if len(set(b[rows])) > 1:
            names.add("conv_tile_crosses_image")
        for k0 in range(0, K, GT_BK):
            taps = sorted({kk // C for kk in range(k0, min(k0 + GT_BK, K), 8)})
            pad_hit = False
            for tap in taps:
                ky, kx = tap // k, tap % k
                iy, ix = oy[rows] * s - p + ky, ox[rows] * s - p + kx
                pad_hit = pad_hit or bool(((iy < 0) | (iy >= H) | (ix < 0) | (ix >= W)).any())
            names.add("conv_tile_with_padding_taps" if pad_hit else "conv_interior_tile")
            if len(taps) > 1:
                names.add("conv_k_tile_straddles_taps")
    if K % GT_BK:
        names.add("conv_ragged_last_k_tile")
    if M % GT_BM:
        names.add("conv_ragged_last_row_tile")
    if M > GT_BM:
        names.add("conv_rows>128")
    if c["O"] % GT_BN:
        names.add("conv_ragged_last_column_tile")
    names.add("conv_epi_" + EPI_NAMES[c["epi"]])
    names.add("conv_y_" + c["cdt"])
    if c["rdt"]:
        names.add("conv_R_" + c["rdt"])
    names.add("conv_C=%d" % C)
    return sorted(names)


# =====================================================================================================================
# inputs
# =====================================================================================================================
def place(x, ld, off=0, guard_rows=0, fill=NAN):
    """x [rows, cols] inside a flat buffer of off + (rows + guard_rows) * ld elements of `fill`; -> (flat, window [rows + guard_rows, ld])"""
    rows, cols = x.shape
    flat = torch.full((off + (rows + guard_rows) * ld,), fill, dtype=x.dtype)
    win = flat[off:].view(rows + guard_rows, ld)
    win[:rows, :cols] = x
    return flat, win


def operand(x, trans, pad):
    """storage of a logical [rows, K] operand: k-contiguous [rows, ld] (zero-padded to K rounded up to 8, NaN beyond) or, trans,
    contraction-major [K, ld] (columns rows..ld NaN).  -> (storage 2-D, ld)"""
    rows, K = x.shape
    if not trans:
        ld = up(K, 8) + pad
        _, win = place(x, ld)
        win[:, K:up(K, 8)] = 0
        return win, ld
    ld = up(rows, 8) + pad
    _, win = place(x.t().contiguous(), ld)
    return win, ld


GUARD_ROWS = 2


def gemm_inputs(cfg, n_cu=DEFAULT_CUS):
    """CPU tensors of a case.  a / b: logical [M, K] and [N, K] in the operand encoding; A / B: their storage; bias, R, C0 (the
    value C holds before an accumulating call) logical."""
    M, N, K = cfg["M"], cfg["N"], cfg["K"]
    g = torch.Generator().manual_seed(cfg["seed"] * 7919 + 13)
    dt = DT[cfg["dt"]]
    a = torch.randn((M, K), generator=g)
    b = torch.randn((N, K), generator=g) / math.sqrt(K)
    if cfg["edge4"]:
        a[:, slab_edges(cfg, n_cu)] *= 4.0
    a, b = a.to(dt), b.to(dt)
    A, lda = operand(a, cfg["ta"], cfg["a_pad"])
    B, ldb = operand(b, cfg["tb"], cfg["b_pad"])
    t = dict(a=a, b=b, A=A, B=B, lda=lda, ldb=ldb)
    t["bias"] = torch.randn((N,), generator=g) * 0.5
    if cfg["epi"] in NEED_R:
        t["R"] = (torch.randn((M, N), generator=g) * (1.5 if cfg["epi"] == EPI_DGELU else 1.0)).to(DT[cfg["rdt"]])
    t["C0"] = torch.randn((M, N), generator=g) if cfg["accumulate"] else None
    return t


def conv_inputs(c):
    Ho, Wo, M, K = conv_dims(c)
    g = torch.Generator().manual_seed(c["seed"] * 7919 + 17)
    x = torch.randn((c["B"], c["H"], c["W"], c["C"]), generator=g)
    w = torch.randn((c["O"], c["k"], c["k"], c["C"]), generator=g) / math.sqrt(K)
    if c["edge4"]:
        w[:, 0, 0, :8] *= 4.0
        w[:, -1, -1, -8:] *= 4.0
    t = dict(x=x.bfloat16(), w=w.bfloat16(), bias=torch.randn((c["O"],), generator=g) * 0.5)
    if c["rdt"]:
        t["R"] = torch.randn((M, c["O"]), generator=g).to(DT[c["rdt"]])
    return t


# =====================================================================================================================
# references and bounds (torch float64, on whatever device the inputs are)
# =====================================================================================================================
def gelu64(z):
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))


def keep_mask(p_drop, key, M, N, device="cpu"):
    """(keep [M, N] float64 of 0 / 1, the f32 scale of the survivors) -- mv_make_drop and the pair mask over index m * N + n"""
    thr = dm_threshold(p_drop)
    inv = float(np.float32(65536.0) / (np.float32(65536.0) - np.float32(thr)))
    return torch.from_numpy(dm_restated(p_drop, key, M * N).astype(np.float64)).view(M, N).to(device), inv


def enc_bound(ref, bound, enc):
    """what storing in `enc` adds to `bound`"""
    if enc == F32:
        return bound
    b = bound + HALF_ULP_REL[enc] * (ref.abs() + bound)
    return b + F16_SUBNORMAL_HALF_ULP if enc == F16 else b


def epilogue_reference(cfg, y, S, slabs, K, bias=None, R=None, C0=None):
    """y = A.B and S = |A|.|B| in float64 -> dict name -> (reference, bound) for C, C2, C3 and the value `pre` that C3 would hold were it
    written before the activation.  All before the output encodings except through enc_bound."""
    e0 = sum_bound(K + slabs, S)
    epi = cfg["epi"]
    rnd = EPI_ROUNDINGS * U32
    out = {}
    if cfg["alpha"] is not None:
        al = f32r(cfg["alpha"])
        y, e0 = y * al, e0 * abs(al) + rnd * (y * al).abs()
    if epi in NEED_BIAS:
        z = y + bias
        ez = e0 + rnd * (y.abs() + bias.abs())
    else:
        z, ez = y, e0
    pre = z
    if epi in (EPI_NONE, EPI_BIAS):
        c, ec = z, ez
        if C0 is not None:
            c, ec = z + C0, ez + rnd * (z.abs() + C0.abs())
    elif epi == EPI_BIAS_GELU:
        out["C2"] = (z, ez)
        c, ec = gelu64(z), LIP_GELU * ez + GELU_TOL * (1 + z.abs())
    elif epi == EPI_BIAS_GELU_D:
        out["C2"] = (dgelu64(z), LIP_DGELU * ez + DACT_TOL)
        c, ec = gelu64(z), LIP_GELU * ez + GELU_TOL * (1 + z.abs())
    elif epi == EPI_BIAS_RES:
        if cfg["p_drop"] > 0:
            keep, inv = keep_mask(cfg["p_drop"], cfg["drop_key"], cfg["M"], cfg["N"], y.device)
            z, ez = z * keep * inv, ez * keep * inv
        c, ec = z + R, ez + rnd * (z.abs() + R.abs())
        pre = c
    elif epi == EPI_RES:
        c, ec = z + R, ez + rnd * (z.abs() + R.abs())
        pre = c
    elif epi == EPI_MUL:
        c, ec = z * R, ez * R.abs() + rnd * (z * R).abs()
        pre = c
    elif epi == EPI_DGELU:
        d = dgelu64(R)
        c, ec = z * d, ez * d.abs() + (z.abs() + ez) * DACT_TOL + rnd * (z * d).abs()
        pre = c
    elif epi == EPI_BIAS_TANH:
        c, ec = torch.tanh(z), ez + TANH_TOL
    elif epi == EPI_BIAS_RELU:
        c, ec = torch.clamp(z, min=0), ez
    elif epi == EPI_BIAS_RES_RELU:
        pre = z + R
        c, ec = torch.clamp(pre, min=0), ez + rnd * (z.abs() + R.abs())
    out["C"] = (c, ec)
    out["pre"] = (pre, ec)
    return out


def gemm_reference(cfg, t, pl, device="cpu"):
    """fp64 references and element-wise bounds of every output of a case (after the output encodings).
    -> dict: C, C2, C3 -> (ref, bound); csum -> (ref [2 * ceil(M / 256), N], bound); colsum -> (ref [N], bound)"""
    a, b = t["a"].to(device).double(), t["b"].to(device).double()
    y, S = a @ b.t(), a.abs() @ b.abs().t()
    bias = t["bias"].to(device).double()
    R = t["R"].to(device).double() if "R" in t else None
    C0 = t["C0"].to(device).double() if t["C0"] is not None else None
    raw = epilogue_reference(cfg, y, S, pl["slabs"], cfg["K"], bias, R, C0)
    out = {"C": (raw["C"][0], enc_bound(*raw["C"], cfg["cdt"]))}
    if "C2" in raw:
        out["C2"] = (raw["C2"][0], enc_bound(*raw["C2"], cfg["cdt"]))
    if cfg["c3dt"]:
        out["C3"] = (raw["C"][0], enc_bound(*raw["C"], cfg["c3dt"]))
        out["C3_pre"] = raw["pre"][0]
    if cfg["csum"]:
        c, ec = raw["C"]
        M, N = cfg["M"], cfg["N"]
        P = 2 * cdiv(M, 256)
        pad = torch.zeros((P * 128 - M, N), dtype=torch.float64, device=c.device)
        halves = lambda x: torch.cat([x, pad]).view(P, 128, N)                  # noqa: E731
        out["csum"] = (halves(c).sum(1), halves(ec).sum(1) + sum_bound(128, halves(c.abs()).sum(1)))
        out["colsum"] = (c.sum(0), ec.sum(0) + sum_bound(128, c.abs().sum(0)) + sum_bound(P, halves(c).sum(1).abs().sum(0)))
    return out


def conv_reference(c, t, device="cpu"):
    Ho, Wo, M, K = conv_dims(c)
    x = t["x"].to(device).double().permute(0, 3, 1, 2)
    w = t["w"].to(device).double().permute(0, 3, 1, 2)
    y = F.conv2d(x, w, stride=c["s"], padding=c["p"]).permute(0, 2, 3, 1).reshape(M, c["O"])
    S = F.conv2d(x.abs(), w.abs(), stride=c["s"], padding=c["p"]).permute(0, 2, 3, 1).reshape(M, c["O"])
    cfg = dict(epi=c["epi"], alpha=None, p_drop=0.0)
    raw = epilogue_reference(cfg, y, S, 1, K, t["bias"].to(device).double(), t["R"].to(device).double() if "R" in t else None, None)
    return {"C": (raw["C"][0], enc_bound(*raw["C"], c["cdt"]))}


def conv_by_loops(c, t):
    """independent formulation of the convolution: explicit loops over the taps of the NHWC tensors, float64"""
    Ho, Wo, M, K = conv_dims(c)
    x, w = t["x"].double(), t["w"].double()
    y = torch.zeros((c["B"], Ho, Wo, c["O"]), dtype=torch.float64)
    for ky in range(c["k"]):
        for kx in range(c["k"]):
            for oy in range(Ho):
                iy = oy * c["s"] - c["p"] + ky
                if iy < 0 or iy >= c["H"]:
                    continue
                for ox in range(Wo):
                    ix = ox * c["s"] - c["p"] + kx
                    if 0 <= ix < c["W"]:
                        y[:, oy, ox, :] += x[:, iy, ix, :] @ w[:, ky, kx, :].t()
    return y.reshape(M, c["O"])


def function_grid():
    """operands of the K = 8 product whose f32 result z[i, j] = (i / 16) (1 + j / 128) is exact: a [257, 8], b [128, 8] (bf16-exact), z fp64"""
    a = torch.zeros((257, 8))
    b = torch.zeros((128, 8))
    a[:, 0] = torch.arange(-128, 129).float() / 16
    b[:, 0] = 1 + torch.arange(128).float() / 128
    return a.bfloat16(), b.bfloat16(), a[:, :1].double() @ b[:, :1].double().t()


def within(got, ref, bound):
    """-> (ok, worst |got - ref| / bound); a non-finite result is never inside"""
    r = (got.double() - ref).abs() / (bound + 1e-300)
    worst = float(r.max()) if r.numel() else 0.0
    return bool(torch.isfinite(got).all()) and worst <= 1.0, worst


# =====================================================================================================================
# the honest f32 computation and the planted defects (CPU): what the bounds must let through and what they must catch
# =====================================================================================================================
DEFECTS = ("alpha", "kchunk", "rgroup", "bias_strip", "c3_pre", "tap")


def defect_applies(defect, cfg):
    if cfg["fam"] == "conv":
        return defect == "kchunk" or (defect == "tap" and cfg["p"] > 0)
    if defect == "alpha":
        return cfg["alpha"] is not None
    if defect == "kchunk":
        return True
    if defect == "rgroup":
        return cfg["epi"] in NEED_R and cfg["M"] >= 48
    if defect == "bias_strip":
        return cfg["epi"] in NEED_BIAS and cfg["N"] >= 2 * STRIP
    if defect == "c3_pre":
        return cfg["c3dt"] is not None and cfg["epi"] in ACTIVATED
    return False


def f32_epilogue(cfg, y, bias, R, C0, defect=None):
    """the epilogue in plain f32 torch -> dict C, C2, C3 (f32 values before the output encodings) and the raw f32 for csum"""
    epi = cfg["epi"]
    if cfg["alpha"] is not None and defect != "alpha":
        y = y * torch.tensor(cfg["alpha"], dtype=torch.float32)
    if R is not None:
        R = R.float()
        if defect == "rgroup":
            R = R.clone()
            R[16:32] = R[32:48]
    if epi in NEED_BIAS:
        bb = bias.clone()
        if defect == "bias_strip":
            bb[:STRIP] = bias[STRIP:2 * STRIP]
        z = y + bb
    else:
        z = y
    out = {}
    pre = z
    if epi in (EPI_NONE, EPI_BIAS):
        c = z if C0 is None else z + C0
    elif epi == EPI_BIAS_GELU:
        out["C2"] = z
        c = F.gelu(z)
    elif epi == EPI_BIAS_GELU_D:
        out["C2"] = dgelu64(z.double()).float()
        c = F.gelu(z)
    elif epi == EPI_BIAS_RES:
        if cfg["p_drop"] > 0:
            keep, inv = keep_mask(cfg["p_drop"], cfg["drop_key"], cfg["M"], cfg["N"])
            z = z * keep.float() * torch.tensor(inv, dtype=torch.float32)
        c = pre = z + R
    elif epi == EPI_RES:
        c = pre = z + R
    elif epi == EPI_MUL:
        c = pre = z * R
    elif epi == EPI_DGELU:
        c = pre = z * dgelu64(R.double()).float()
    elif epi == EPI_BIAS_TANH:
        c = torch.tanh(z)
    elif epi == EPI_BIAS_RELU:
        c = torch.clamp(z, min=0)
    else:
        pre = z + R
        c = torch.clamp(pre, min=0)
    out["C"] = c
    out["C3"] = pre if defect == "c3_pre" else c
    return out


def honest_gemm(cfg, t, pl, defect=None):
    """mv_gemm of a case in plain f32 torch on the CPU (slab by slab when it splits), outputs rounded to their encodings"""
    a, b = t["a"].float(), t["b"].float()
    if defect == "kchunk":
        a = a.clone()
        hi = min(cfg["K"], pl["kchunk"])
        a[:, max(hi - 8, 0):hi] = 0                       # the last 8-element chunk of the first slab
    y = torch.zeros((cfg["M"], cfg["N"]))
    for s in range(pl["slabs"]):
        lo, hi = s * pl["kchunk"], min(cfg["K"], (s + 1) * pl["kchunk"])
        y = y + a[:, lo:hi] @ b[:, lo:hi].t()
    raw = f32_epilogue(cfg, y, t["bias"], t.get("R"), t["C0"], defect)
    out = {"C": raw["C"].to(DT[cfg["cdt"]])}
    if "C2" in raw:
        out["C2"] = raw["C2"].to(DT[cfg["cdt"]])
    if cfg["c3dt"]:
        out["C3"] = raw["C3"].to(DT[cfg["c3dt"]])
    if cfg["csum"]:
        P = 2 * cdiv(cfg["M"], 256)
        out["csum"] = torch.cat([raw["C"], torch.zeros((P * 128 - cfg["M"], cfg["N"]))]).view(P, 128, cfg["N"]).sum(1)
        out["colsum"] = out["csum"].sum(0)
    return out


def conv_patches(c, t, unchecked_tap=None):
    """the [M, K] patch matrix gathered from the flat NHWC buffer, f32; unchecked_tap: that (ky, kx) is read without its padding test
    (the address arithmetic of stage_load_conv then lands on another pixel of the buffer)"""
    Ho, Wo, M, K = conv_dims(c)
    k, s, p, H, W, C, B = c["k"], c["s"], c["p"], c["H"], c["W"], c["C"], c["B"]
    flat = t["x"].float().reshape(B * H * W, C)
    m = torch.arange(M)
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    cols = []
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy * s - p + ky, ox * s - p + kx
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            pix = (b * H * W + iy * W + ix) % (B * H * W)
            v = flat[pix]
            if (ky, kx) != unchecked_tap:
                v = v * ok[:, None].float()
            cols.append(v)
    return torch.cat(cols, dim=1)


def honest_conv(c, t, defect=None):
    Ho, Wo, M, K = conv_dims(c)
    pm = conv_patches(c, t, (0, 0) if defect == "tap" else None)
    if defect == "kchunk":                                # the first 8 channels of the centre tap (inside the image for every row)
        k0 = ((c["k"] // 2) * c["k"] + c["k"] // 2) * c["C"]
        pm[:, k0:k0 + 8] = 0
    y = pm @ t["w"].float().reshape(c["O"], K).t()
    cfg = dict(epi=c["epi"], alpha=None, p_drop=0.0)
    raw = f32_epilogue(cfg, y, t["bias"], t.get("R"), None, None)
    return {"C": raw["C"].to(DT[c["cdt"]])}


# =====================================================================================================================
# census
# =====================================================================================================================
FAMILIES = {
    "small": small_cases, "ring": ring_cases, "pring_walk": pring_cases, "valu": valu_cases, "auto": auto_cases, "reduce": reduce_cases,
    "workspace": workspace_cases, "epi": epi_cases, "conv": conv_cases,
}


def branches(cfg, n_cu=DEFAULT_CUS):
    return conv_branches(cfg) if cfg["fam"] == "conv" else plan(cfg, n_cu)["branches"]


def census(fam):
    count = {}
    for c in FAMILIES[fam]():
        for b in branches(c):
            count[b] = count.get(b, 0) + 1
    return count


def all_gemm_cases():
    return [c for f, gen in FAMILIES.items() if f != "conv" for c in gen()]
