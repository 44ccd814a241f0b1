"""Case generators, dispatch predicates, fp64 references and error bounds of the decode-kernel sweep (csrc/mv_decode.hip).

Plain module in the shape of tests/rowops_cases.py: nothing here touches the GPU or the HIP library.  tests/test_decode_fuzz_gpu.py
runs the cases, tests/test_decode_cases_cpu.py counts which branch every case takes and checks the constants below against the
.hip source.

* every generator draws from np.random.RandomState(fixed + seed) and returns a dict; the tensors of a case are made from that dict
  alone, so a cfg printed by a failing assertion reproduces the case;
* next to every generator stands a restatement of the launcher's / kernel's dispatch arithmetic, which names the branches a case takes;
* the references are plain torch in float64 (CPU or device tensors); none of them calls a kernel of this project.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from rowops_cases import BF16, DT, ESIZE, F16, F16_SUBNORMAL_HALF_ULP, F32, LN_CONST_ROW_VALUE, U16, U32, f32r, out16_bound, rowrel, sum_bound, up  # noqa: F401

# ---- constants of csrc/mv_decode.hip (tests/test_decode_cases_cpu.py reads the same numbers out of the source) -------------------
GR_WAVES = 4
GR_BN = 16
GR_U = 4                      # weight fragments in flight per wave: the unroll of the contraction loop
GR_MAX_M = 256
GR_KSTEP = 32                 # one MFMA 16x16x32 step of the contraction
AD_TILE = 256                 # keys per tile = threads per block
AD_MAX_DH = 128
AD_SPLIT_BLOCKS = 512         # decode_splits: blocks wanted
AD_SPLIT_MIN_KEYS = 128       # decode_splits: keys per split at least
AD_SPLIT_MAX = 32
TK_THREADS = 256
TK_MAX_K = 16
TK_KM = ((1, 1), (4, 4), (16, 16))       # (largest k, list length KM) in dispatch order
TK_EOS_LOGPROB = -10000.0
ER_MAX_H = 8192

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_BIAS_RELU = 0, 1, 2, 3, 9       # include/medvill.h
EPI_NAME = {EPI_NONE: "epi_none", EPI_BIAS: "epi_bias", EPI_BIAS_GELU: "epi_bias_gelu", EPI_BIAS_RES: "epi_bias_res", EPI_BIAS_RELU: "epi_bias_relu"}

# ---- tolerances the fixed-shape tests of tests/test_generate_gpu.py assert for the same kernels --------------------------------
AD_TOL = {F32: 2e-5, BF16: 2e-2, F16: 3e-3}
TK_TOL = 1e-4
ER_TOL = 1e-5                 # mv_embed_rows has no fixed-shape test: the LayerNorm forward figure of the row-kernel sweep
CPU_FACTOR = 4.0              # a case's tolerance is never below 4 x the error of plain f32 torch on the CPU on the same inputs


def gr_flat_tol(K, out_is_f32):
    """test_gemm_rows_matches_matmul's absolute tolerance"""
    return 2e-3 * math.sqrt(K / 768) + (0.0 if out_is_f32 else 4e-2)


def store16_bound(ref, enc, f32_abs):
    """a value within f32_abs (absolute, scalar or element-wise) of ref in f32, then stored once in a 16-bit encoding"""
    return out16_bound(ref, enc, 0.0) + f32_abs


def case_tol(base, cpu_f32, ref64):
    """the larger of the fixed-shape tolerance and CPU_FACTOR x the largest absolute error plain f32 torch on the CPU makes against
    fp64 on the same inputs.  Never measured from the kernel under test."""
    d = (cpu_f32.double() - ref64).abs()
    d = d[torch.isfinite(ref64)]
    return max(base, CPU_FACTOR * float(d.max())) if d.numel() else base


# =====================================================================================================================
# mv_gemm_rows
# =====================================================================================================================
GR_M = (1, 15, 16, 17, 37, 255, 256)
GR_N = (1, 3, 16, 17, 464, 768, 1000)
GR_N_VOCAB = 30522
GR_K = (32, 64, 96, 128, 160, 256, 768, 3072)
GR_GUARD_ROWS = 2             # rows of the output allocation before and after the logical [M, ldc] block
N_GR = 96


def gr_wave_steps(K):
    """contraction steps of the four waves of a block"""
    n = K // GR_KSTEP
    return [(w + 1) * n // GR_WAVES - w * n // GR_WAVES for w in range(GR_WAVES)]


def gr_c_start(cfg):
    """element offset of C[0, 0] inside its (16-byte aligned) allocation"""
    return GR_GUARD_ROWS * cfg["ldc"] + cfg["c_off"]


def gr_branches(cfg):
    M, N, K = cfg["M"], cfg["N"], cfg["K"]
    b = ["mt=%d" % ((M + 15) // 16), "ops_" + cfg["ops"], "c_" + cfg["cdt"], EPI_NAME[cfg["epi"]]]
    if cfg["epi"] == EPI_BIAS_RES:
        b.append("res_" + cfg["rdt"])
        if cfg["rdt"] != cfg["ops"]:
            b.append("res_cross_encoded")
        if cfg["ldr"] > N:
            b.append("ldr>N")
    for name, ld, n in (("ldx>K", cfg["ldx"], K), ("ldw>K", cfg["ldw"], K), ("ldc>N", cfg["ldc"], N)):
        if ld > n:
            b.append(name)
    if M % 16:
        b.append("M%16!=0")
    if M == GR_MAX_M:
        b.append("M=256")
    if N < GR_BN:
        b.append("N<16")
    if N % GR_BN:
        b.append("N%16!=0")
    if N % 4:
        b.append("N%4!=0")
    # a full group of 4 columns is stored as one vector when its address is a multiple of 4 elements (16 bytes f32, 8 bytes 16-bit)
    if N >= 4:
        al = {(gr_c_start(cfg) + m * cfg["ldc"]) % 4 == 0 for m in range(min(M, 4))}
        if True in al:
            b.append("store_vector")
        if False in al:
            b.append("store_scalar_misaligned")
    steps = gr_wave_steps(K)
    if K // GR_KSTEP < GR_WAVES:
        b.append("wave_empty")
    if any(0 < s < GR_U for s in steps):
        b.append("wave_tail_only")
    if any(s >= GR_U and s % GR_U for s in steps):
        b.append("wave_unrolled+tail")
    if any(s >= GR_U and s % GR_U == 0 for s in steps):
        b.append("wave_unrolled_only")
    return b


def gr_case(seed):
    rs = np.random.RandomState(8000 + seed)
    mt = seed % 16 + 1
    M = int((16 * mt - 15, 16 * mt - 1, 16 * mt, 16 * mt - 11)[(seed // 16 + seed) % 4])
    N = int(GR_N[seed % len(GR_N)])
    K = int(GR_K[(seed + seed // 8) % len(GR_K)])
    epi = (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_BIAS_RELU, EPI_BIAS_RES)[(seed + seed // 6) % 6]
    return dict(fam="gr", seed=seed, M=M, N=N, K=K, ops=(BF16, F16)[rs.randint(2)], cdt=(F32, BF16, F16)[(seed // 2) % 3], epi=epi,
                rdt=(F32, BF16, F16)[(seed // 6) % 3], ldx=K + int(rs.choice([0, 8, 40])), ldw=K + int(rs.choice([0, 8, 24])),
                ldc=N + int(rs.choice([0, 0, 1, 3, 4, 8])), c_off=int(rs.randint(3) == 0), ldr=N + int(rs.choice([0, 3, 8])))


GR_FIXED = [
    # the MLM head's own width, kept to a few cases: a classifier-sized batch, the full 256 rows on a one-step contraction, one row
    dict(fam="gr", seed=9801, M=37, N=GR_N_VOCAB, K=768, ops=BF16, cdt=F32, epi=EPI_BIAS, rdt=F32, ldx=768, ldw=768, ldc=30528, c_off=0, ldr=GR_N_VOCAB),
    dict(fam="gr", seed=9802, M=256, N=GR_N_VOCAB, K=32, ops=F16, cdt=F16, epi=EPI_NONE, rdt=F32, ldx=40, ldw=32, ldc=30523, c_off=0, ldr=GR_N_VOCAB),
    dict(fam="gr", seed=9803, M=1, N=GR_N_VOCAB, K=3072, ops=F16, cdt=F32, epi=EPI_BIAS_RES, rdt=BF16, ldx=3072, ldw=3080, ldc=GR_N_VOCAB, c_off=1, ldr=30525),
    dict(fam="gr", seed=9804, M=37, N=464, K=768, ops=F16, cdt=F32, epi=EPI_BIAS_RELU, rdt=F32, ldx=768, ldw=768, ldc=464, c_off=0, ldr=464),
    dict(fam="gr", seed=9805, M=255, N=17, K=96, ops=BF16, cdt=BF16, epi=EPI_BIAS_GELU, rdt=F32, ldx=104, ldw=96, ldc=17, c_off=1, ldr=17),
    dict(fam="gr", seed=9806, M=256, N=1000, K=3072, ops=BF16, cdt=F32, epi=EPI_BIAS_RES, rdt=F16, ldx=3072, ldw=3072, ldc=1003, c_off=0, ldr=1000),
    dict(fam="gr", seed=9807, M=17, N=3, K=64, ops=F16, cdt=F16, epi=EPI_BIAS_RES, rdt=F32, ldx=64, ldw=72, ldc=3, c_off=0, ldr=6),
]


def gr_cases():
    return [gr_case(s) for s in range(N_GR)] + GR_FIXED


def gr_inputs(cfg):
    """CPU tensors: x [M, ldx] and W [N, ldw] in the operand encoding, bias f32 [N], res [M, ldr] in its encoding.  The padding columns
    of x, W and res hold NaN: a read past K or past N shows in the result."""
    M, N, K = cfg["M"], cfg["N"], cfg["K"]
    g = torch.Generator().manual_seed(cfg["seed"])
    x = torch.full((M, cfg["ldx"]), float("nan"))
    x[:, :K] = torch.randn((M, K), generator=g)
    W = torch.full((N, cfg["ldw"]), float("nan"))
    W[:, :K] = torch.randn((N, K), generator=g) * 0.05
    bias = torch.randn((N,), generator=g) * 0.1
    res = torch.full((M, cfg["ldr"]), float("nan"))
    res[:, :N] = torch.randn((M, N), generator=g)
    return x.to(DT[cfg["ops"]]), W.to(DT[cfg["ops"]]), bias, res.to(DT[cfg["rdt"]])


def gr_reference(x64, W64, bias64, res64, epi):
    """x64 [M, K], W64 [N, K], bias64 [N], res64 [M, N], all fp64.  -> (epi(x W^T), pre-activation, sum_k |x_k w_k|)"""
    z = x64 @ W64.t()
    s_abs = x64.abs() @ W64.abs().t()
    if epi != EPI_NONE:
        z = z + bias64
    if epi == EPI_BIAS_GELU:
        out = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    elif epi == EPI_BIAS_RELU:
        out = torch.clamp(z, min=0.0)
    elif epi == EPI_BIAS_RES:
        out = z + res64
    else:
        out = z
    return out, z, s_abs


def gr_linear_bound(K, s_abs, bias64, res64, epi):
    """Element-wise f32 bound of the epilogues without a transcendental: the K-term sum in any order (sum_bound) plus one rounding
    for the bias add and one for the residual add, each relative to at most the magnitudes that enter it.  ReLU is 1-Lipschitz."""
    b = sum_bound(K, s_abs)
    if epi != EPI_NONE:
        b = b + U32 * (s_abs + bias64.abs())
    if epi == EPI_BIAS_RES:
        b = b + U32 * (s_abs + bias64.abs() + res64.abs())
    return b


def gr_f32_cpu(x, W, bias, res, epi):
    """the same product in plain f32 torch (F.linear and the epilogue) on the CPU"""
    z = F.linear(x.float(), W.float(), None if epi == EPI_NONE else bias.float())
    if epi == EPI_BIAS_GELU:
        return F.gelu(z)
    if epi == EPI_BIAS_RELU:
        return F.relu(z)
    if epi == EPI_BIAS_RES:
        return z + res.float()
    return z


# =====================================================================================================================
# mv_attn_decode
# =====================================================================================================================
AD_DH = (4, 8, 16, 32, 64, 128)
AD_A = (1, 2, 3, 12)
AD_R = (1, 2, 5, 24)
AD_COLS = (100, 300, 1100)          # width of the slot table = largest key count of the case
AD_S = 1500                         # cache rows
AD_PLANT_SLOTS = 8                  # the last cache rows are never drawn: a planted key sits there
AD_NK_EDGES = (0, 1, 256, 257, 1100)
AD_MODES = ("one", "forced", "auto_full", "auto_half", "auto_no_ws", "forced_many")
AD_LATE_SCORE, AD_DOMINANT_SCORE = 6.0, 12.0
AD_GUARD_ROWS = 2
N_AD = 96


def decode_splits(R, A, dh, max_nk, ws_floats):
    """the library's split choice, restated"""
    pairs = R * A
    s = (AD_SPLIT_BLOCKS + pairs - 1) // pairs
    s = min(s, max(1, (max_nk + AD_SPLIT_MIN_KEYS - 1) // AD_SPLIT_MIN_KEYS))
    s = min(s, AD_SPLIT_MAX)
    while s > 1 and s * pairs * (dh + 2) > ws_floats:
        s -= 1
    return max(s, 1)


def ad_nk(cfg):
    """key counts of the R query rows: drawn in 1..cols, the edge values the case carries written over the first rows, and the last
    row at the full width when a key is planted in it"""
    rs = np.random.RandomState(8150 + cfg["seed"])
    nk = rs.randint(1, cfg["cols"] + 1, size=cfg["R"]).astype(np.int32)
    for i, v in enumerate(cfg["edges"][:cfg["R"]]):
        nk[(i + cfg["seed"]) % cfg["R"]] = v
    if cfg["plant"] or int(nk.max()) == 0:
        nk[cfg["R"] - 1] = cfg["cols"]
    return nk


def ad_plan(cfg):
    """-> dict(nk, max_nk, nsplit argument, ws_floats, splits that run, splits the library would pick with unlimited workspace)"""
    R, A, dh = cfg["R"], cfg["A"], cfg["dh"]
    nk = ad_nk(cfg)
    max_nk = max(1, int(nk.max()))
    pairs = R * A
    free = decode_splits(R, A, dh, max_nk, 1 << 60)
    mode = cfg["mode"]
    if mode == "one":
        arg, ws_floats = 1, 0
    elif mode in ("forced", "forced_many"):
        arg = cfg["nsplit"]
        ws_floats = arg * pairs * (dh + 2)
    elif mode == "auto_full":
        arg, ws_floats = 0, AD_SPLIT_MAX * pairs * (dh + 2)
    elif mode == "auto_half":
        arg, ws_floats = 0, max(1, free // 2) * pairs * (dh + 2) + 1
    else:
        arg, ws_floats = 0, 0
    ns = decode_splits(R, A, dh, max_nk, ws_floats) if arg == 0 else arg
    return dict(nk=nk, max_nk=max_nk, nsplit=arg, ws_floats=ws_floats, ns=ns, free=free)


def ad_plant_pos(cfg, plan):
    """(query row, position in its key list) of the planted key, or None"""
    if not cfg["plant"]:
        return None
    r = cfg["R"] - 1
    n, ns = int(plan["nk"][r]), plan["ns"]
    chunk = (n + ns - 1) // ns
    if cfg["plant"] == "late":
        return r, min(chunk, n) - 1              # the last key of split 0
    return r, n - 1                              # "dominate": the last key of the last split that owns keys


def ad_branches(cfg):
    plan = ad_plan(cfg)
    nk, ns, R, A, dh = plan["nk"], plan["ns"], cfg["R"], cfg["A"], cfg["dh"]
    H = A * dh
    b = ["dt_" + cfg["dt"], "dh=%d" % dh, "A=%d" % A]
    if plan["nsplit"] == 1:
        b.append("nsplit=1")
    elif plan["nsplit"] > 1:
        b.append("nsplit>1")
    else:
        b.append("auto->1" if ns == 1 else "auto->many")
        if plan["ws_floats"] == 0:
            b.append("auto_no_ws")
        elif ns < plan["free"]:
            b.append("auto_capped_by_ws")
    b.append("slot_row_shared" if cfg["shared"] else "slot_row_none")
    for v in (0, 1, 256, 257):
        if (nk == v).any():
            b.append("nk=%d" % v)
    if (nk > 1024).any():
        b.append("nk>1024")
    if any((ns - 1) * ((int(n) + ns - 1) // ns) >= int(n) for n in nk if n > 0) and ns > 1:
        b.append("empty_split")
    pp = ad_plant_pos(cfg, plan)
    if pp is not None:
        n = int(nk[pp[0]])
        chunk = (n + ns - 1) // ns
        if cfg["plant"] == "late" and pp[1] - (pp[1] // chunk) * chunk >= AD_TILE:
            b.append("max_rises_in_later_tile")
        if cfg["plant"] == "dominate" and ns > 1 and chunk < n:
            b.append("one_split_dominates")
    if cfg["dup"] and (nk >= 4).any():
        b.append("duplicate_slots")
    if cfg["ldq"] > H:
        b.append("ldq>H")
    if cfg["ldkv"] > H:
        b.append("ldkv>H")
    if cfg["ldo"] > H:
        b.append("ldo>H")
    return b


def ad_case(seed):
    rs = np.random.RandomState(8100 + seed)
    dh = int(AD_DH[seed % len(AD_DH)])
    A = int(AD_A[(seed + seed // 6) % len(AD_A)])
    H = A * dh
    mode = AD_MODES[(seed + seed // 12) % len(AD_MODES)]
    R = int(AD_R[rs.randint(len(AD_R))])
    cols = int(AD_COLS[(seed // 3) % len(AD_COLS)])
    plant = (None, "late", "dominate")[seed % 3]
    if plant == "late":
        mode, cols = ("one", "auto_no_ws", "forced")[(seed // 3) % 3], 1100
    if plant == "dominate" and mode in ("one", "auto_no_ws"):
        mode = "forced"
    edges = tuple(v for v in np.roll(AD_NK_EDGES, seed).tolist() if v <= cols)
    nsplit = int(rs.choice([2, 3, 8])) if mode == "forced" else (int(rs.choice([5, 16, 32])) if mode == "forced_many" else 0)
    if plant == "late":
        nsplit = 2 if mode == "forced" else nsplit       # 550 keys per split: the planted key sits in the split's third tile
    return dict(fam="ad", seed=seed, dt=(F32, BF16, F16)[(seed // 6) % 3], dh=dh, A=A, R=R, cols=cols, mode=mode, nsplit=nsplit, edges=edges,
                shared=bool(R >= 2 and rs.randint(2)), plant=plant, dup=bool(rs.randint(2)),
                ldq=int(rs.choice([H, 3 * H])), ldkv=int(rs.choice([H, 2 * H, H + 4])), ldo=int(rs.choice([H, H + 4, 3 * H])))


def ad_cases():
    return [ad_case(s) for s in range(N_AD)]


def ad_inputs(cfg):
    """CPU tensors of a case.  -> dict(q [R, ldq] (query in the first H columns, NaN behind), k / v [S, ldkv] (NaN padding; with
    ldkv = 2H one fused tensor, v = its second half), slots int32 [rows, cols], slot_row int32 [R] or None, nk int32 [R], plan)"""
    R, A, dh, cols = cfg["R"], cfg["A"], cfg["dh"], cfg["cols"]
    H, dt = A * dh, DT[cfg["dt"]]
    plan = ad_plan(cfg)
    g = torch.Generator().manual_seed(cfg["seed"])
    q = torch.full((R, cfg["ldq"]), float("nan"))
    q[:, :H] = torch.randn((R, H), generator=g)
    q = q.to(dt)
    kk = torch.randn((AD_S, H), generator=g)
    vv = torch.randn((AD_S, H), generator=g)
    rows = (R + 1) // 2 if cfg["shared"] else R
    slots = torch.randint(0, AD_S - AD_PLANT_SLOTS, (rows, cols), generator=g, dtype=torch.int32)
    if cfg["dup"] and cols > 3:
        slots[:, 3] = slots[:, 0]
        slots[:, cols - 1] = slots[:, 0]
    slot_row = (torch.arange(R, dtype=torch.int32) // 2) if cfg["shared"] else None
    pp = ad_plant_pos(cfg, plan)
    if pp is not None:
        r, pos = pp
        score = AD_LATE_SCORE if cfg["plant"] == "late" else AD_DOMINANT_SCORE
        slots[int(slot_row[r]) if slot_row is not None else r, pos] = AD_S - 1
        qr = q[r, :H].float().view(A, dh)
        kk[AD_S - 1] = (qr * (score * math.sqrt(dh) / (qr * qr).sum(dim=1, keepdim=True).clamp_min(1e-3))).reshape(-1)
    if cfg["ldkv"] == 2 * H:
        kv = torch.cat([kk, vv], dim=1).to(dt)
        k, v = kv, kv[:, H:]
    else:
        k = torch.full((AD_S, cfg["ldkv"]), float("nan"))
        v = torch.full((AD_S, cfg["ldkv"]), float("nan"))
        k[:, :H], v[:, :H] = kk, vv
        k, v = k.to(dt), v.to(dt)
    return dict(q=q, k=k, v=v, slots=slots, slot_row=slot_row, nk=torch.from_numpy(plan["nk"].copy()), plan=plan)


def ad_reference(q, k, v, slots, slot_row, nk, A, dh, dtype=torch.float64):
    """gather + softmax + weighted sum per (row, head) in `dtype`; a row without keys is zero.  q [R, >=H], k / v [S, >=H] (any
    encoding, the first H columns count).  -> [R, H]"""
    R, H = q.shape[0], A * dh
    out = torch.zeros((R, H), dtype=dtype, device=q.device)
    for r in range(R):
        n = int(nk[r])
        if n == 0:
            continue
        s = slots[int(slot_row[r]) if slot_row is not None else r, :n].long()
        kr = k[s][:, :H].to(dtype).view(n, A, dh)
        vr = v[s][:, :H].to(dtype).view(n, A, dh)
        qq = q[r, :H].to(dtype).view(A, dh)
        p = torch.softmax(torch.einsum("ad,jad->aj", qq, kr) / math.sqrt(dh), dim=-1)
        out[r] = torch.einsum("aj,jad->ad", p, vr).reshape(-1)
    return out


def ad_reference_split_merge(q, k, v, slots, slot_row, nk, A, dh, ns):
    """independent formulation in fp64: the key list cut in ns chunks of ceil(n / ns), every chunk walked in tiles of AD_TILE keys
    with a running (max, sum, context), the chunks merged through their maxima, written out with loops.
    -> ([R, H], number of tiles that raised a running maximum after the first tile of their chunk)"""
    R, H = q.shape[0], A * dh
    out = torch.zeros((R, H), dtype=torch.float64)
    rises = 0
    for r in range(R):
        n = int(nk[r])
        sl = slots[int(slot_row[r]) if slot_row is not None else r]
        chunk = (n + ns - 1) // ns
        for h in range(A):
            qq = q[r, h * dh:(h + 1) * dh].double() / math.sqrt(dh)
            parts = []
            for sp in range(ns):
                j0, j1 = sp * chunk, min(n, sp * chunk + chunk)
                m, l, acc = -math.inf, 0.0, torch.zeros(dh, dtype=torch.float64)
                for jt in range(j0, j1, AD_TILE):
                    s = sl[jt:min(jt + AD_TILE, j1)].long()
                    sc = k[s][:, h * dh:(h + 1) * dh].double() @ qq
                    m_new = max(m, float(sc.max()))
                    rises += int(jt > j0 and m_new > m)
                    p = torch.exp(sc - m_new)
                    corr = math.exp(m - m_new) if m > -math.inf else 0.0
                    l = l * corr + float(p.sum())
                    acc = acc * corr + p @ v[s][:, h * dh:(h + 1) * dh].double()
                    m = m_new
                parts.append((m, l, acc))
            big = max(p[0] for p in parts) if parts else -math.inf
            if big > -math.inf:
                l = sum(p[1] * math.exp(p[0] - big) for p in parts if p[0] > -math.inf)
                o = sum(p[2] * math.exp(p[0] - big) for p in parts if p[0] > -math.inf)
                out[r, h * dh:(h + 1) * dh] = o / l
    return out, rises


# =====================================================================================================================
# mv_logprob_topk
# =====================================================================================================================
TK_V = (1, 2, 40, 255, 256, 257, 1000, 30522)
TK_V_EXTRA = (3, 5, 8, 16)               # k == V under the longer lists (KM = 4, 16) needs vocabularies the value set above lacks
TK_K = (1, 2, 3, 4, 5, 8, 15, 16)
TK_GRID = 2.0 ** -8                      # every logit is a multiple of it
TK_RANGE = 2048                          # ordinary draws: multiples in [-8, 8]
TK_TOP = 9.0                             # planted values sit above every ordinary draw
TK_LARGE = 80.0
TK_EOS_BEST = 90.0
TK_PAD_LOGIT = 3.0e4                     # columns V..ld-1: read as a logit it would be every row's maximum
TK_ROWS = ("plain", "tie_same_thread", "tie_same_wave", "tie_other_wave", "row_all_equal", "topk_all_in_one_thread_stride",
           "neg_inf_in_first_256", "neg_inf_elsewhere", "large_magnitude")
TK_EOS_MODES = ("eos_none", "eos_penalised", "eos_out_of_range", "eos_was_best", "eos_in_tie")
TK_GUARD_ROWS = 2
TK_IDX_SENTINEL = -(2 ** 40) - 12345
N_TK = 96


def tk_km(k):
    for kmax, km in TK_KM:
        if k <= kmax:
            return km
    raise ValueError(k)


def tk_row_kinds(cfg):
    """what is planted in each of the rows of a case: the kinds of TK_ROWS the vocabulary and k have room for, 'plain' otherwise"""
    V, k = cfg["V"], cfg["k"]
    ok = {"plain": True, "tie_same_thread": V > TK_THREADS, "tie_same_wave": V >= 2, "tie_other_wave": V > 64, "row_all_equal": True,
          "topk_all_in_one_thread_stride": k >= 2 and V > TK_THREADS * (k - 1), "neg_inf_in_first_256": V >= 2,
          "neg_inf_elsewhere": V > TK_THREADS, "large_magnitude": True}
    return [kind if ok[kind] else "plain" for kind in TK_ROWS]


def tk_eos(cfg):
    """the eos_penalty_id argument"""
    V, mode = cfg["V"], cfg["eos_mode"]
    if mode == "eos_none":
        return -1
    if mode == "eos_out_of_range":
        return (V, V + 3, 2 ** 30)[cfg["seed"] % 3]
    return int(np.random.RandomState(8250 + cfg["seed"]).randint(V))


def tk_branches(cfg):
    """The launch-level names from the cfg; what the rows hold (ties, -inf, the penalised column's standing) from the logits themselves
    and the reference's selection (tk_observed), so that a plant another plant has overwritten is not counted."""
    V, k = cfg["V"], cfg["k"]
    x64 = tk_inputs(cfg)[:, :V].double()
    obs = tk_observed(cfg, x64, tk_reference(x64, k, tk_eos(cfg))[1])
    mode = cfg["eos_mode"]
    b = ["km%d" % tk_km(k), mode if mode in obs or mode in TK_EOS_MODES[:3] else "eos_penalised", "lse_out" if cfg["lse_out"] else "lse_absent"]
    if k == V:
        b.append("k==V")
        if "eos_selected" in obs:
            b.append("eos_enters_because_k==V")
    if V < TK_THREADS:
        b.append("idle_threads")
    if cfg["ld"] > V:
        b.append("ld>V_padding_larger_than_max")
    b += sorted(n for n in obs if n in TK_ROWS)
    return b


def tk_case(seed):
    rs = np.random.RandomState(8200 + seed)
    V = int(TK_V[seed % len(TK_V)]) if seed % 12 != 11 else int(TK_V_EXTRA[(seed // 12) % len(TK_V_EXTRA)])
    ks = [k for k in TK_K if k <= V] + ([V] if V <= TK_MAX_K else [])
    k = int(ks[(seed // 8 + seed) % len(ks)])
    if V in TK_V_EXTRA:
        k = V
    return dict(fam="tk", seed=seed, V=V, k=k, ld=int((V, V + 1, up(V, 8) + 8)[rs.randint(3)]), eos_mode=TK_EOS_MODES[(seed + seed // 5) % 5],
                lse_out=bool(seed % 3))


TK_FIXED = [
    # the MLM head's row: vocabulary 30522 in rows of 30528, the widths beam search asks for
    dict(fam="tk", seed=9851, V=30522, k=16, ld=30528, eos_mode="eos_was_best", lse_out=True),
    dict(fam="tk", seed=9852, V=30522, k=5, ld=30528, eos_mode="eos_in_tie", lse_out=False),
    dict(fam="tk", seed=9853, V=30522, k=15, ld=30522, eos_mode="eos_penalised", lse_out=True),
    dict(fam="tk", seed=9854, V=1000, k=3, ld=1001, eos_mode="eos_in_tie", lse_out=True),
    dict(fam="tk", seed=9855, V=16, k=16, ld=16, eos_mode="eos_in_tie", lse_out=True),
    dict(fam="tk", seed=9856, V=257, k=2, ld=264, eos_mode="eos_none", lse_out=True),
]


def tk_cases():
    return [tk_case(s) for s in range(N_TK)] + TK_FIXED


def tk_inputs(cfg):
    """CPU f32 logits [rows, ld]: multiples of TK_GRID, padding columns at TK_PAD_LOGIT, one planted feature per row (tk_row_kinds)."""
    V, k, ld = cfg["V"], cfg["k"], cfg["ld"]
    kinds = tk_row_kinds(cfg)
    rs = np.random.RandomState(8300 + cfg["seed"])
    x = rs.randint(-TK_RANGE, TK_RANGE + 1, size=(len(kinds), V)).astype(np.float64) * TK_GRID
    for i, kind in enumerate(kinds):
        if kind == "tie_same_thread":
            c = int(rs.randint(V - TK_THREADS))
            x[i, [c, c + TK_THREADS]] = TK_TOP
            if c + 2 * TK_THREADS < V:
                x[i, c + 2 * TK_THREADS] = TK_TOP
        elif kind == "tie_same_wave":
            c = int(rs.randint(V - 1))
            c -= int(c % 64 == 63)
            x[i, [c, c + 1]] = TK_TOP
        elif kind == "tie_other_wave":
            c = int(rs.randint(V - 64))
            x[i, [c, c + 64]] = TK_TOP
            if c + 192 < V:
                x[i, c + 192] = TK_TOP
        elif kind == "row_all_equal":
            x[i] = -1.0
        elif kind == "topk_all_in_one_thread_stride":
            c0 = int(rs.randint(min(TK_THREADS, V - TK_THREADS * (k - 1))))
            x[i, c0 + TK_THREADS * np.arange(k)] = TK_TOP + rs.permutation(k) * TK_GRID
        elif kind == "neg_inf_in_first_256":
            w = min(V, TK_THREADS)
            cols = rs.permutation(w)[:max(1, min(w // 4, V - 1))]
            if cfg["seed"] % 2 and V > 1:
                cols[0] = 0                           # the very first column a thread sees, thread 0 included
            x[i, cols] = -np.inf
        elif kind == "neg_inf_elsewhere":
            cols = TK_THREADS + rs.permutation(V - TK_THREADS)[:max(1, (V - TK_THREADS) // 8)]
            x[i, cols] = -np.inf
        elif kind == "large_magnitude":
            x[i] = np.where(rs.rand(V) < 0.5, TK_LARGE, -TK_LARGE) + rs.randint(-512, 513, size=V) * TK_GRID
    eos = tk_eos(cfg)
    if cfg["eos_mode"] == "eos_was_best":
        x[:, eos] = TK_EOS_BEST
    elif cfg["eos_mode"] == "eos_in_tie" and V > 1:
        others = np.delete(x, eos, axis=1).max(axis=1)
        x[:, eos] = np.where(np.isfinite(others), others, x[:, eos])
    out = np.full((len(kinds), ld), TK_PAD_LOGIT)
    out[:, :V] = x
    return torch.from_numpy(out).float()


def tk_reference(x64, k, eos):
    """x64 fp64 [R, V] -> (vals fp64 [R, k], idx int64 [R, k], lse fp64 [R]): log-softmax, the penalised column at -10000 exactly,
    a stable sort by (value descending, column ascending).  A -inf logit adds nothing to the sum and ranks last, by column."""
    V = x64.shape[1]
    lse = torch.logsumexp(x64, dim=-1)
    lp = x64 - lse[:, None]
    if 0 <= eos < V:
        lp[:, eos] = TK_EOS_LOGPROB
    order = torch.sort(-lp, dim=-1, stable=True).indices[:, :k]
    return lp.gather(1, order), order, lse


def tk_reference_by_hand(x64, k, eos):
    """independent formulation: log_softmax from the library, the order from numpy's lexsort on (column, -value)"""
    V = x64.shape[1]
    lp = torch.log_softmax(x64, dim=-1).numpy().copy()
    if 0 <= eos < V:
        lp[:, eos] = TK_EOS_LOGPROB
    idx = np.stack([np.lexsort((np.arange(V), -row))[:k] for row in lp])
    lse = np.log(np.exp(x64.numpy() - x64.numpy().max(axis=1, keepdims=True)).sum(axis=1)) + x64.numpy().max(axis=1)
    return torch.from_numpy(np.take_along_axis(lp, idx, axis=1)), torch.from_numpy(idx), torch.from_numpy(lse)


def tk_f32_cpu(x, k, eos):
    """plain f32 torch on the CPU: (log-probabilities of the reference's columns are gathered by the caller) -> (lp f32 [R, V], lse f32)"""
    lp = torch.log_softmax(x.float(), dim=-1)
    if 0 <= eos < x.shape[1]:
        lp[:, eos] = TK_EOS_LOGPROB
    return lp, torch.logsumexp(x.float(), dim=-1)


def tk_observed(cfg, x64, idx):
    """what the rows of a case really contain, from its logits x64 [R, V] and the reference's selection idx [R, k] (names as tk_branches)"""
    V, k = cfg["V"], cfg["k"]
    eos = tk_eos(cfg)
    pen = 0 <= eos < V
    seen = set()
    xs = x64.numpy()
    for i in range(xs.shape[0]):
        row, sel = xs[i], [int(c) for c in idx[i]]
        for a in sel:
            if pen and a == eos:
                continue
            same = [int(c) for c in np.flatnonzero(row == row[a]) if c != a and not (pen and c == eos)]
            for c in same:
                if c % TK_THREADS == a % TK_THREADS:
                    seen.add("tie_same_thread")
                elif (c % TK_THREADS) // 64 == (a % TK_THREADS) // 64:
                    seen.add("tie_same_wave")
                else:
                    seen.add("tie_other_wave")
        if np.all(row == row[0]):
            seen.add("row_all_equal")
        if k >= 2 and len({c % TK_THREADS for c in sel}) == 1:
            seen.add("topk_all_in_one_thread_stride")
        ninf = np.flatnonzero(np.isneginf(row))
        if len(ninf) and ninf.min() < TK_THREADS:
            seen.add("neg_inf_in_first_256")
        if len(ninf) and ninf.max() >= TK_THREADS:
            seen.add("neg_inf_elsewhere")
        if np.isfinite(row).any() and np.abs(row[np.isfinite(row)]).max() >= TK_LARGE - 2:
            seen.add("large_magnitude")
        if pen:
            if int(np.argmax(row)) == eos:
                seen.add("eos_was_best")
            if any(row[c] == row[eos] for c in sel if c != eos):
                seen.add("eos_in_tie")
            if eos in sel:
                seen.add("eos_selected")
    return seen


# =====================================================================================================================
# mv_embed_rows
# =====================================================================================================================
ER_H = (4, 100, 256, 260, 768, 1024, 8192)
ER_R = (1, 3, 64, 272)
ER_OOB = ("none", "id<0", "id>=V", "pos<0", "pos>=maxpos", "seg<0", "seg>=ntype", "none")
ER_V, ER_MAXPOS = 11, 7
ER_CONST = dict(id=1, pos=1)          # table rows that hold constants; the constant row's segment is ntype - 1
ER_GUARD_ROWS = 2
N_ER = 84


def er_kinds(cfg):
    """per query row: which index is out of its table ('none': all inside)"""
    return [ER_OOB[(r + cfg["seed"]) % len(ER_OOB)] for r in range(cfg["R"])]


def er_const_row(cfg):
    """the query row whose three table rows are constants (sum LN_CONST_ROW_VALUE), or None"""
    if not cfg["const"]:
        return None
    kinds = er_kinds(cfg)
    inside = [r for r in range(cfg["R"]) if kinds[r] == "none"]
    return inside[cfg["seed"] % len(inside)] if inside else None


def er_branches(cfg):
    b = ["dt_" + cfg["dt"], "ntype=%d" % cfg["ntype"], "eps=%g" % cfg["eps"]]
    if cfg["ldo"] > cfg["H"]:
        b.append("ldo>H")
    if cfg["H"] % 256:
        b.append("H%256!=0")
    if cfg["H"] < 256:
        b.append("idle_threads")
    b += sorted({k for k in er_kinds(cfg) if k != "none"})
    if er_const_row(cfg) is not None:
        b.append("constant_row")
    return b


def er_case(seed):
    rs = np.random.RandomState(8400 + seed)
    H = int(ER_H[seed % len(ER_H)])
    R = int(ER_R[(seed + seed // 7) % len(ER_R)])
    return dict(fam="er", seed=seed, dt=(F32, BF16, F16)[(seed // 2) % 3], H=H, R=R, ldo=H + int(rs.choice([0, 4, 1, 36])), ntype=1 + (seed // 3) % 2,
                eps=(1e-12, 1e-5)[(seed // 4) % 2], const=bool(seed % 4 != 3))


def er_cases():
    return [er_case(s) for s in range(N_ER)]


def er_inputs(cfg):
    """CPU tensors: ids / pos / seg int64 [R] (some outside their tables, er_kinds), E [V, H], P [maxpos, H], Ty [ntype, H] in the
    encoding (dense), gamma / beta f32 [H].  -> dict"""
    R, H, nt = cfg["R"], cfg["H"], cfg["ntype"]
    g = torch.Generator().manual_seed(cfg["seed"])
    rs = np.random.RandomState(8450 + cfg["seed"])
    E = torch.randn((ER_V, H), generator=g)
    P = torch.randn((ER_MAXPOS, H), generator=g) * 0.5
    Ty = torch.randn((nt, H), generator=g) * 0.5
    E[ER_CONST["id"]] = 1.0
    P[ER_CONST["pos"]] = 0.25
    gamma = torch.randn((H,), generator=g) * 0.1 + 1.0
    beta = torch.randn((H,), generator=g) * 0.1
    ids, pos, seg = rs.randint(0, ER_V, R), rs.randint(0, ER_MAXPOS, R), rs.randint(0, nt, R)
    far = (1, 5, 2 ** 31, 2 ** 40, 2 ** 62)
    for r, kind in enumerate(er_kinds(cfg)):
        f = int(far[(r + cfg["seed"]) % len(far)])
        if kind == "id<0":
            ids[r] = -f
        elif kind == "id>=V":
            ids[r] = ER_V - 1 + f
        elif kind == "pos<0":
            pos[r] = -f
        elif kind == "pos>=maxpos":
            pos[r] = ER_MAXPOS - 1 + f
        elif kind == "seg<0":
            seg[r] = -f
        elif kind == "seg>=ntype":
            seg[r] = nt - 1 + f
    const = er_const_row(cfg)
    if const is not None:
        Ty[nt - 1] = LN_CONST_ROW_VALUE - 1.25
        ids[const], pos[const], seg[const] = ER_CONST["id"], ER_CONST["pos"], nt - 1
    dt = DT[cfg["dt"]]
    return dict(ids=torch.from_numpy(ids.astype(np.int64)), pos=torch.from_numpy(pos.astype(np.int64)), seg=torch.from_numpy(seg.astype(np.int64)),
                E=E.to(dt), P=P.to(dt), Ty=Ty.to(dt), gamma=gamma, beta=beta, const=const)


def er_sum(ids, pos, seg, E, P, Ty, dtype):
    """E[id] + Ty[seg] + P[pos] with the indices clamped into their tables, as the ABI defines them"""
    i = ids.clamp(0, E.shape[0] - 1)
    p = pos.clamp(0, P.shape[0] - 1)
    t = seg.clamp(0, Ty.shape[0] - 1)
    return E.to(dtype)[i] + Ty.to(dtype)[t] + P.to(dtype)[p]


def er_reference(ids, pos, seg, E, P, Ty, gamma, beta, eps, dtype=torch.float64):
    x = er_sum(ids, pos, seg, E, P, Ty, dtype)
    return F.layer_norm(x, (x.shape[1],), gamma.to(dtype), beta.to(dtype), eps)


def er_reference_closed_form(ids, pos, seg, E, P, Ty, gamma, beta, eps):
    """independent formulation: the clamp written with min / max per row, LayerNorm in closed form"""
    rows = []
    for r in range(ids.shape[0]):
        i = min(max(int(ids[r]), 0), E.shape[0] - 1)
        p = min(max(int(pos[r]), 0), P.shape[0] - 1)
        t = min(max(int(seg[r]), 0), Ty.shape[0] - 1)
        rows.append(E[i].double() + Ty[t].double() + P[p].double())
    x = torch.stack(rows)
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


# =====================================================================================================================
# census
# =====================================================================================================================
FAMILIES = {
    "gr": (gr_cases, gr_branches),
    "ad": (ad_cases, ad_branches),
    "tk": (tk_cases, tk_branches),
    "er": (er_cases, er_branches),
}


def census(fam):
    """branch name -> number of cases of the family that reach it"""
    cases, branches = FAMILIES[fam]
    count = {}
    for c in cases():
        for b in branches(c):
            count[b] = count.get(b, 0) + 1
    return count
