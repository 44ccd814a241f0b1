"""Case generators, dispatch predicates and fp64 references of the row-kernel sweep (csrc/mv_rowops.hip).

Plain module: nothing here touches the GPU or the HIP library.  tests/test_rowops_fuzz_gpu.py runs the cases, and
tests/test_rowops_cases_cpu.py counts which launcher branch every case takes, so that a retuned cap or a changed draw cannot
quietly turn the sweep into a no-op.

* every generator draws from np.random.RandomState(fixed + seed) and returns a dict; the tensors of a case are then made from
  cfg["seed"] alone (torch.Generator().manual_seed), so a cfg printed by a failing assertion reproduces the case;
* next to every generator stands a restatement of the launcher's dispatch conditions, which names the branch(es) a case takes;
* the references are plain torch in float64 (CPU or device tensors); none of them calls a kernel of this project.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16, F16 = "f32", "bf16", "f16"
DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
ESIZE = {F32: 4, BF16: 2, F16: 2}
# unit roundoff of a value stored in the encoding: half an ulp relative to the value.  (bf16's is taken relative to the value
# plus the row maximum, see out16_bound, which is never below half a bf16 ulp of the value.)
U16 = {BF16: 2.0 ** -9, F16: 2.0 ** -11}
F16_SUBNORMAL_HALF_ULP = 2.0 ** -25          # below 2^-14 an f16 rounds to multiples of 2^-24, whatever its size
U32 = 2.0 ** -24

# ---- caps and thresholds of the launchers (tests/test_rowops_cases_cpu.py reads the same numbers out of the .hip source) -----------
CE_SCALAR8_MAX_V = 2048          # V <= 2048: ce_kernel<., ., 8>; above it the vector kernel or ce_kernel<., ., 128>
CE_VEC_MAX = 32768               # vector kernel: V and ldd <= 1024 * 32
CE_VEC_ROWS = 512                # vector kernel: at most 512 blocks, a block walks rows beyond that
CE_MAX_V = 256 * 128
LN_MAX_H = 2048
LN_NC_STEPS = (256, 768, 1024)   # NC_DISPATCH: 1, 3, 4 chunks of 256 columns up to these widths, else 8
LN_BWD_CAPS = {0: 512, 3: 256, 1: 1024, 2: 1024}
LN_BWD_WPB = {0: 8, 3: 16, 1: 4, 2: 4}
LN_WIDE_MAX_H = 768
COLSUM_BLOCKS = 2048
PARTIALS_BLOCKS = 512
ELEMWISE_BLOCKS = 2048           # mv_add, mv_dact, mv_cast, mv_count_nonfinite: blocks of 256 threads x 4 elements
ADAMW_BLOCKS = 4096
DROPMASK_BLOCKS = 4096
CAST2D_ROWS_PER_LAUNCH = 65535
CAST2D_COL_BLOCKS = 32

ELEMWISE_SPAN = ELEMWISE_BLOCKS * 256 * 4
ADAMW_SPAN = ADAMW_BLOCKS * 256 * 4


def up(n, k):
    return (n + k - 1) // k * k


def f32r(x):
    """the value a C float argument holds"""
    return float(np.float32(x))


# =====================================================================================================================
# error bounds
# =====================================================================================================================
def sum_bound(n_terms, sum_abs):
    """Standard bound of an n-term f32 summation in any order: |err| <= 2 n 2^-24 sum|terms| (sum_abs from the fp64 reference)."""
    return 2.0 * n_terms * U32 * sum_abs


def out16_bound(ref, enc, f32_tol):
    """Element-wise bound of a value computed in f32 and stored in a 16-bit encoding: half an ulp of the encoding on top of the f32
    tolerance of the same kernel (f32_tol, relative to the row's largest magnitude, as the f32 tests state it).  The half ulp is taken
    as U16 times (|value| + the row's largest magnitude): the second term is the floor that keeps entries near zero from dominating,
    and it also makes the bound at least 2^-8 |value| for bf16, whose unit roundoff is 2^-8 (U16 holds 2^-9).  f16 adds its
    subnormal quantum 2^-25: below 2^-14 an f16 rounds to multiples of 2^-24 whatever its size.  ref: fp64 [rows, cols]."""
    rowmax = ref.abs().amax(dim=-1, keepdim=True)
    b = U16[enc] * (ref.abs() + rowmax) + f32_tol * rowmax
    if enc == F16:
        b = b + F16_SUBNORMAL_HALF_ULP
    return b


def rowrel(got, ref):
    """largest error of a row relative to that row's largest reference magnitude (not below 1e-3 of the global one), over rows"""
    ref = ref.detach()
    rowmax = ref.abs().amax(dim=-1, keepdim=True)
    den = torch.maximum(rowmax, 1e-3 * ref.abs().max()) + 1e-300
    return float(((got.double() - ref).abs() / den).max())


# =====================================================================================================================
# cross-entropy
# =====================================================================================================================
CE_V = (2, 5, 1000, 2048, 2049, 2050, 30522, 32768)
CE_R = (1, 37, 511, 513, 1500)
CE_PAIRS = ((F32, F32), (F32, F16), (F32, BF16), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, None), (BF16, None), (F16, None))
CE_LDD_WIDE = 32772
N_CE = 72


def ce_branch(cfg):
    """mv_ce_fwd_bwd: which kernel a case runs.  -> (branch, reasons the vector kernel was refused)"""
    V, R, ld, has_d = cfg["V"], cfg["R"], cfg["ld"], cfg["ddt"] is not None
    ldd = cfg["ldd"] if has_d else 0
    l_aligned = (cfg["l_off"] * ESIZE[cfg["ldt"]]) % 16 == 0
    d_aligned = (not has_d) or (cfg["d_off"] * ESIZE[cfg["ddt"]]) % 16 == 0
    why = []
    if ld % 4:
        why.append("ld%4")
    if has_d and ldd % 4:
        why.append("ldd%4")
    if not l_aligned:
        why.append("logits_misaligned")
    if not d_aligned:
        why.append("dlogits_misaligned")
    if ldd > CE_VEC_MAX:
        why.append("ldd>32768")
    vec_ok = not why and V > CE_SCALAR8_MAX_V and V <= CE_VEC_MAX
    if vec_ok:
        return ("vec_rowwalk" if R > CE_VEC_ROWS else "vec"), []
    if V <= 256 * 8:
        return "scalar8", why
    return "scalar128", why


def ce_branches(cfg):
    """the kernel a case runs plus what it carries into it (for the census)"""
    br, why = ce_branch(cfg)
    b = [br] + ["scalar128:" + w for w in why if br == "scalar128"]
    b.append("logits_" + cfg["ldt"])
    b.append("dlogits_" + (cfg["ddt"] or "absent"))
    if cfg["ties"] and cfg["R"] >= 6:
        b.append("ties_same_vector+other_wave+last_column")       # ce_inputs cycles the three placements over the tied rows
    if br.startswith("vec") and cfg["V"] % 4 and cfg["R"] >= 37:
        b.append("label_in_padded_last_vector")                   # 15 % of the rows are labelled V - 1
    b.append("labels_" + cfg["labels"])
    b.append("scale_" + cfg["scale"])
    return b


def ce_wave_step(branch):
    """column distance that moves a logit into another wave's share of the row (scalar: thread = c % 256; vector: (c / 4) % 1024)"""
    return 256 if branch.startswith("vec") else 64


def ce_case(seed):
    rs = np.random.RandomState(7000 + seed)
    V = int(CE_V[seed % len(CE_V)] if seed < 2 * len(CE_V) else rs.choice(CE_V))
    R = int(rs.choice(CE_R if V < 30000 else (1, 37, 511, 513)))       # the 1500-row batch at vocabulary width is a fixed case
    ldt, ddt = CE_PAIRS[rs.randint(len(CE_PAIRS))]
    ld = int(rs.choice([V, V + 1, up(V, 4), up(V, 8)]))
    ldd = int(rs.choice([V, V + 1, up(V, 4), up(V, 8), CE_LDD_WIDE])) if ddt else 0
    if ldd == CE_LDD_WIDE and R > 513:
        R = 513
    # a base one element off 16-byte alignment is safe to pass: hip_ops hands the kernel tensor.data_ptr() as it is, the launcher tests
    # that address (vec_ok) and falls back to ce_kernel, which touches logits and gradient through ldf / stf only (mv_common.h:
    # one element per access)
    mis = int(rs.randint(4))                 # 0, 1: aligned | 2: logits base one element off | 3: gradient base one element off
    ties = seed % 3 != 1                     # two thirds of the cases force ties for the maximum
    labels = ["mixed", "mixed", "mixed", "mixed", "mixed", "oob", "oob", "all_ignored"][rs.randint(8)]
    scale = ["host", "dev", "host_x_loss"][seed % 3]
    return dict(fam="ce", seed=seed, V=V, R=R, ldt=ldt, ddt=ddt, ld=ld, ldd=ldd, l_off=1 if mis == 2 else 0,
                d_off=1 if (mis == 3 and ddt) else 0, ties=ties, labels=labels, scale=scale)


CE_FIXED = [
    # the MLM head's own shape: vocabulary 30522 padded to 30528, more rows than the vector kernel has blocks
    dict(fam="ce", seed=9001, V=30522, R=1500, ldt=BF16, ddt=BF16, ld=30528, ldd=30528, l_off=0, d_off=0, ties=True, labels="mixed", scale="dev"),
    # 128 logits per thread, rows of 30522 with an odd leading dimension
    dict(fam="ce", seed=9002, V=30522, R=513, ldt=F32, ddt=F32, ld=30523, ldd=30522, l_off=0, d_off=0, ties=True, labels="mixed", scale="host"),
    dict(fam="ce", seed=9003, V=32768, R=37, ldt=F16, ddt=F16, ld=32768, ldd=32768, l_off=0, d_off=1, ties=True, labels="oob", scale="host_x_loss"),
    dict(fam="ce", seed=9004, V=2049, R=513, ldt=F32, ddt=BF16, ld=2052, ldd=CE_LDD_WIDE, l_off=0, d_off=0, ties=True, labels="mixed", scale="dev"),
    dict(fam="ce", seed=9005, V=2050, R=1500, ldt=F16, ddt=F32, ld=2052, ldd=2052, l_off=0, d_off=0, ties=True, labels="mixed", scale="host"),
    dict(fam="ce", seed=9006, V=30522, R=37, ldt=F32, ddt=F32, ld=30524, ldd=30524, l_off=0, d_off=0, ties=False, labels="all_ignored", scale="host"),
]


def ce_cases():
    return [ce_case(s) for s in range(N_CE)] + CE_FIXED


def ce_inputs(cfg):
    """CPU tensors of a case: logits [R, V] (already in the logit encoding), labels int64 [R] and, per row, the tied columns."""
    V, R = cfg["V"], cfg["R"]
    g = torch.Generator().manual_seed(cfg["seed"])
    rs = np.random.RandomState(7500 + cfg["seed"])
    x = (torch.randn((R, V), generator=g) * 2.0).to(DT[cfg["ldt"]])
    lab = torch.from_numpy(rs.randint(0, V, size=R)).long()
    lab[torch.from_numpy(rs.rand(R) < 0.15)] = V - 1
    lab[torch.from_numpy(rs.rand(R) < 0.10)] = 0
    step = ce_wave_step(ce_branch(cfg)[0])
    tie_rows = {}
    if cfg["ties"] and V > 1:
        for j, i in enumerate(range(cfg["seed"] % 2, R, 2)):
            c0 = int(x[i].float().argmax())
            mode = ("same_vec", "other_wave", "last")[j % 3]
            if mode == "same_vec":
                grp = [c for c in range(c0 // 4 * 4, min(c0 // 4 * 4 + 4, V)) if c != c0]
                first = grp[rs.randint(len(grp))] if grp else (c0 + 1) % V
            elif mode == "other_wave":
                first = c0 + step if c0 + step < V else (c0 - step if c0 - step >= 0 else (c0 + 1) % V)
            else:
                first = V - 1 if c0 != V - 1 else 0
            cols = {c0, first}
            for _ in range(int(rs.randint(3))):
                cols.add(int(rs.randint(V)))
            cols = sorted(cols)
            x[i, cols] = x[i, c0].clone()
            tie_rows[i] = (mode, cols)
            lab[i] = cols[0] if j % 2 == 0 else cols[-1]       # the first tied column is the argmax; the last one is not
    lab[torch.from_numpy(rs.rand(R) < 0.2)] = -100
    if cfg["labels"] == "all_ignored":
        lab[:] = -100
    elif cfg["labels"] == "oob":
        oob = torch.from_numpy(rs.rand(R) < 0.3)
        lab[oob] = torch.from_numpy(rs.choice([V, V + 7, 2 ** 31 - 1], size=R)).long()[oob]
        lab[0] = V                                              # at least one, also when R == 1
    return x, lab, tie_rows


def ce_scales(cfg):
    """(grad_scale on the device or None, grad_scale on the host, loss scale on the device or None, the product)"""
    R = cfg["R"]
    if cfg["scale"] == "dev":
        return 0.125, 777.0, None, 0.125                       # the device value wins over the host argument
    if cfg["scale"] == "host":
        return None, f32r(1.0 / R), None, f32r(1.0 / R)
    return None, f32r(1.0 / R), 1024.0, f32r(1.0 / R) * 1024.0


def first_argmax(x):
    """index of the first maximum of every row, written out (no reliance on a library's tie rule)"""
    V = x.shape[-1]
    idx = torch.arange(V, device=x.device).expand_as(x)
    mx = x.amax(dim=-1, keepdim=True)
    return torch.where(x == mx, idx, torch.full_like(idx, V)).amin(dim=-1)


def ce_reference(x64, lab, scale):
    """x64: fp64 [R, V]; lab int64 [R] (any value outside 0..V-1 = ignored row, the kernel's documented behaviour).
    -> (nll sum, labelled rows, argmax hits, gradient fp64 [R, V])"""
    V = x64.shape[1]
    valid = (lab >= 0) & (lab < V)
    lab_t = torch.where(valid, lab, torch.full_like(lab, -100))
    xg = x64.detach().clone().requires_grad_(True)
    nll = F.cross_entropy(xg, lab_t, ignore_index=-100, reduction="sum")
    (nll * scale).backward()
    hits = int(((first_argmax(x64) == lab) & valid).sum())
    return float(nll.detach()), int(valid.sum()), hits, xg.grad


def ce_reference_by_hand(x64, lab):
    """independent formulation: -(log_softmax)[label] summed by hand; gradient softmax - onehot"""
    V = x64.shape[1]
    lse = torch.logsumexp(x64, dim=-1)
    nll, grad = 0.0, torch.zeros_like(x64)
    for i in range(x64.shape[0]):
        li = int(lab[i])
        if 0 <= li < V:
            nll += float(lse[i] - x64[i, li])
            grad[i] = torch.exp(x64[i] - lse[i])
            grad[i, li] -= 1.0
    return nll, grad


# =====================================================================================================================
# LayerNorm
# =====================================================================================================================
LN_H = (4, 100, 256, 260, 764, 768, 772, 1024, 1028, 2044, 2048)
LN_M = (1, 3, 37, 513, 4100)
LN_FWD_PAIRS = ((F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16))                  # (y, x)
LN_BWD_PAIRS = ((F32, F32), (BF16, F32), (BF16, BF16), (BF16, F16), (F16, F32), (F16, F16))     # (dy, x)
N_LN = 96


def ln_nc(H):
    for nc, lim in zip((1, 3, 4), LN_NC_STEPS):
        if H <= lim:
            return nc
    return 8


def ln_fwd_branches(cfg):
    H, M = cfg["H"], cfg["M"]
    b = [f"fwd_nc{ln_nc(H)}", f"fwd_{cfg['ydt']}_from_{cfg['xdt']}"]
    if H % 256:
        b.append("fwd_ragged_last_chunk")
    if cfg["y_bf16"]:
        b.append("fwd_y_bf16")
    if M == 1:
        b.append("M=1")
    if M % 4:
        b.append("fwd_M%4")
    return b


def ln_bwd_plan(cfg):
    """mv_layernorm_bwd: (kernel form that runs, waves per block, blocks, whether a wave walks more than one row)"""
    H, M, var = cfg["H"], cfg["M"], cfg["variant"]
    if var in (0, 3) and not (H <= LN_WIDE_MAX_H and cfg["xdt"] != F32):
        var = 2
    wpb = LN_BWD_WPB[var]
    blocks = min((M + wpb - 1) // wpb, LN_BWD_CAPS[var])
    return var, wpb, blocks, M > blocks * wpb


def ln_bwd_branches(cfg):
    var, wpb, blocks, walks = ln_bwd_plan(cfg)
    b = [{0: "bwd_pf8", 1: "bwd_plain", 2: "bwd_pf4", 3: "bwd_pf16"}[var], f"bwd_nc{ln_nc(cfg['H'])}", f"bwd_{cfg['ddt']}_x_{cfg['xdt']}"]
    if var != cfg["variant"]:
        b.append("bwd_wide_refused")
    if walks:
        b.append("bwd_row_walk")
    if cfg["M"] % wpb:
        b.append("bwd_M%wpb")
    if cfg["H"] % 256:
        b.append("bwd_ragged_last_chunk")
    b.append("bwd_dropout" if cfg["p_drop"] > 0 else "bwd_no_dropout")
    return b


def ln_case(seed):
    rs = np.random.RandomState(7100 + seed)
    H = int(LN_H[seed % len(LN_H)] if seed < 2 * len(LN_H) else rs.choice(LN_H))
    M = int(rs.choice(LN_M))
    xdt = [F32, BF16, F16][rs.randint(3)]
    ydt = str(rs.choice([y for (y, x) in LN_FWD_PAIRS if x == xdt]))
    ddt = str(rs.choice([d for (d, x) in LN_BWD_PAIRS if x == xdt]))
    return dict(fam="ln", seed=seed, H=H, M=M, xdt=xdt, ydt=ydt, ddt=ddt, y_bf16=bool(ydt == F16 and rs.randint(2)),
                variant=int(seed % 4), p_drop=float(rs.choice([0.0, 0.1])), drop_key=int(rs.randint(1, 2 ** 31)),
                eps=float(rs.choice([1e-12, 1e-5])), unscale=float(rs.choice([1.0, 0.25, 1.0 / 1024])))


LN_FIXED = [
    # the wide prefetching blocks walking rows: 16-bit rows of 768 elements, more rows than blocks x waves
    dict(fam="ln", seed=9101, H=768, M=4100, xdt=F16, ydt=F16, ddt=BF16, y_bf16=True, variant=0, p_drop=0.1, drop_key=1234567, eps=1e-12, unscale=1.0 / 1024),
    dict(fam="ln", seed=9102, H=764, M=4100, xdt=BF16, ydt=BF16, ddt=BF16, y_bf16=False, variant=3, p_drop=0.1, drop_key=99, eps=1e-12, unscale=0.25),
    dict(fam="ln", seed=9103, H=2044, M=4100, xdt=F32, ydt=F32, ddt=F32, y_bf16=False, variant=1, p_drop=0.0, drop_key=1, eps=1e-5, unscale=1.0),
    dict(fam="ln", seed=9104, H=260, M=4100, xdt=F16, ydt=F16, ddt=F16, y_bf16=True, variant=2, p_drop=0.1, drop_key=5, eps=1e-12, unscale=1.0),
    dict(fam="ln", seed=9105, H=100, M=1, xdt=F16, ydt=F16, ddt=BF16, y_bf16=True, variant=3, p_drop=0.0, drop_key=5, eps=1e-12, unscale=1.0),
]
LN_CONST_ROW_VALUE = 1.5          # exact in every encoding and in every partial sum: mean exact, variance exactly 0
LN_CONST_ROW_DY_SCALE = 2.0 ** -10   # its rstd is 1 / sqrt(eps), up to 1e6: keeps that row's dx inside f16's range


def ln_cases():
    return [ln_case(s) for s in range(N_LN)] + LN_FIXED


def ln_inputs(cfg):
    """CPU tensors: x (in its encoding; a quarter of the rows sit at an offset of about 100 with a spread of 1, one row is constant),
    gamma, beta (f32), dy (in its encoding).  -> (x, gamma, beta, dy, index of the constant row or None)"""
    M, H = cfg["M"], cfg["H"]
    g = torch.Generator().manual_seed(cfg["seed"])
    x = torch.randn((M, H), generator=g) * 2.0 + 0.5
    off = torch.arange(M) % 4 == 1
    x[off] = torch.randn((int(off.sum()), H), generator=g) + 100.0
    const = (cfg["seed"] * 7) % M if M >= 3 else None       # a batch of one or two rows keeps ordinary rows
    if const is not None:
        x[const] = LN_CONST_ROW_VALUE
    gamma = torch.randn((H,), generator=g) * 0.1 + 1.0
    beta = torch.randn((H,), generator=g) * 0.1
    dy = torch.randn((M, H), generator=g)
    if const is not None:
        dy[const] *= LN_CONST_ROW_DY_SCALE
    return x.to(DT[cfg["xdt"]]), gamma, beta, dy.to(DT[cfg["ddt"]]), const


def ln_reference(x64, gamma64, beta64, dy64, eps):
    """F.layer_norm and its autograd in fp64.  -> dict(y, mean, rstd, dx, dgamma, dbeta, xhat)"""
    H = x64.shape[1]
    xg, gg, bg = (t.detach().clone().requires_grad_(True) for t in (x64, gamma64, beta64))
    y = F.layer_norm(xg, (H,), gg, bg, eps)
    (y * dy64).sum().backward()
    mean = x64.mean(dim=1)
    rstd = 1.0 / torch.sqrt(x64.var(dim=1, unbiased=False) + eps)
    return dict(y=y.detach(), mean=mean, rstd=rstd, dx=xg.grad, dgamma=gg.grad, dbeta=bg.grad,
                xhat=(x64 - mean[:, None]) * rstd[:, None])


def ln_f32_cpu(x, gamma, beta, dy, eps):
    """The same operation in plain f32 torch on the CPU (F.layer_norm and its autograd) on a case's own inputs.  -> (y, dx), f32"""
    xg = x.float().detach().clone().requires_grad_(True)
    y = F.layer_norm(xg, (x.shape[1],), gamma.float(), beta.float(), eps)
    (y * dy.float()).sum().backward()
    return y.detach(), xg.grad


def ln_case_tol(base, cpu_f32, ref64, const=None):
    """Tolerance of one case for an f32 LayerNorm output, in the row-relative measure of rowrel(): the tolerance the fixed-shape tests
    assert (1e-5 forward, 1e-4 backward), or 4 x the error that plain f32 torch on the CPU makes against fp64 on the same inputs,
    whichever is larger.  The rows at an offset of 100 lose log2(100 * rstd) bits when the mean is subtracted, in any f32
    implementation; on the narrow ones (H = 4, where rstd can be large) the CPU itself misses 1e-5: 6.6e-5 at ln seed 0.
    The factor of 4 covers a different summation order.  Never measured from the kernel under test.  The constant row is left out
    of the measurement (its rstd is 1 / sqrt(eps), so whatever the CPU's own variance rounds to would decide the figure)."""
    if const is not None:
        rows = torch.arange(ref64.shape[0], device=ref64.device) != const
        cpu_f32, ref64 = cpu_f32[rows], ref64[rows]
    return max(base, 4.0 * rowrel(cpu_f32.double(), ref64))


LN_XHAT_ROUNDINGS = 8      # dgamma's term dy * xhat: see ln_term_errors
LN_DX_ROUNDINGS = 64


def ln_term_errors(x64, dy64, ref, dd_ref, const):
    """f32 error of ONE term of the column sums of the LayerNorm backward, from its arithmetic, [M, H] each (the sums themselves get
    the summation bound on top).  The backward is fed mean and rstd rounded to f32, so
      xhat = (x - mean) * rstd  is off by at most 2^-24 (|mean| rstd + 3 |xhat|): the rounding of mean, of the difference, of rstd and
      of the product; dgamma's term dy * xhat adds one rounding.  Doubled for slack: LN_XHAT_ROUNDINGS 2^-24 |dy| (max|x| rstd + max|xhat|).
      dx = rstd * (g dy - mean(g dy) - xhat mean(g dy xhat)): two row reductions (at most 32 sequential adds per lane + 6 shuffle
      levels each, every rounding relative to at most the row's largest product) and a handful of element-wise roundings, the xhat
      error above entering through the last product: LN_DX_ROUNDINGS 2^-24 max(1, max|x| rstd / 4) times the row's largest |dx|
      (4 is the size xhat itself reaches).  The constant row cancels exactly (x - mean = 0), so nothing is amplified there.
    dbeta's terms are the inputs themselves: no term error."""
    amp = x64.abs().amax(dim=1, keepdim=True) * ref["rstd"][:, None]
    if const is not None:
        amp[const] = 0.0
    xh_max = ref["xhat"].abs().amax(dim=1, keepdim=True)
    dg = LN_XHAT_ROUNDINGS * U32 * dy64.abs() * (amp + xh_max)
    cs = LN_DX_ROUNDINGS * U32 * (torch.clamp(amp / 4.0, min=1.0) * dd_ref.abs().amax(dim=1, keepdim=True)).expand_as(dy64)
    return {"dg": dg, "db": torch.zeros_like(dy64), "cs": cs}


def ln_bwd_closed_form(x64, gamma64, dy64, eps):
    """the closed form in the header comment of ln_bwd_kernel:
    dx = rstd*(g*dy - mean(g*dy) - xhat*mean(g*dy*xhat)); dgamma = sum dy*xhat; dbeta = sum dy"""
    mean = x64.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    xhat = (x64 - mean) * rstd
    gd = gamma64 * dy64
    dx = rstd * (gd - gd.mean(dim=1, keepdim=True) - xhat * (gd * xhat).mean(dim=1, keepdim=True))
    return dx, (dy64 * xhat).sum(0), dy64.sum(0)


# =====================================================================================================================
# gather / scatter
# =====================================================================================================================
GS_H = (4, 132, 768, 1024, 2048)
GS_R = (1, 2, 5, 41, 1000)
N_GS = 60


def gs_branches(cfg):
    b = [f"{cfg['op']}_{cfg['dt']}"]
    b.append("one_pass" if cfg["H"] <= 256 else ("H>768" if cfg["H"] > 768 else "column_loop"))
    if cfg["H"] % 256:
        b.append("ragged_last_pass")
    if cfg["lds"] != cfg["H"] and cfg["ldd"] != cfg["H"] and cfg["lds"] != cfg["ldd"]:
        b.append("lds!=H!=ldd")
    if cfg["n_neg"]:
        b.append("negative_rows")
    if cfg["R"] % 4:
        b.append("R%4")
    return b


def gs_case(seed):
    rs = np.random.RandomState(7200 + seed)
    H = int(GS_H[seed % len(GS_H)])
    R = int(rs.choice(GS_R))
    pads = [0, 4, 8, 12, 36]
    lds, ldd = H + int(rs.choice(pads)), H + int(rs.choice(pads))
    if seed % 2 and lds == ldd:
        ldd = lds + 4
    n_neg = int(rs.choice([0, 1, 3])) if R > 1 else int(rs.randint(2))
    return dict(fam="gs", seed=seed, op=("gather", "scatter", "scatter_acc")[(seed // len(GS_H)) % 3], dt=[F32, BF16, F16][rs.randint(3)],
                H=H, R=R, lds=lds, ldd=ldd, n_other=R + int(rs.choice([0, 3, 50])), n_neg=min(n_neg, R))


def gs_cases():
    return [gs_case(s) for s in range(N_GS)]


def gs_rows(cfg):
    """R DISTINCT indices into the other side's n_other rows, n_neg of them replaced by negative values"""
    rs = np.random.RandomState(7250 + cfg["seed"])
    rows = rs.permutation(cfg["n_other"])[:cfg["R"]].astype(np.int64)
    neg = rs.permutation(cfg["R"])[:cfg["n_neg"]]
    rows[neg] = rs.choice([-1, -100, -2 ** 31], size=len(neg))
    return torch.from_numpy(rows)


# =====================================================================================================================
# column sums
# =====================================================================================================================
CS_N = (1, 3, 8, 100, 129, 768, 770, 3072, 30522)
CS_M = (1, 7, 255, 257, 5000, 40000)
CS_MAX_ELEMS = 1 << 23           # the random draw keeps M * ldx below this; the one case above it is fixed
N_CS = 90


def cs_plan(cfg):
    """mv_colsum: (column strips, row slices, row slices capped by the block budget)"""
    strip = 128 if cfg["dt"] == F32 else 256
    xb = (cfg["N"] + strip - 1) // strip
    ysplit = (cfg["M"] + 255) // 256
    want = (COLSUM_BLOCKS + xb - 1) // xb
    return xb, max(1, min(ysplit, want)), ysplit > want


def cs_branches(cfg):
    vec_w = 16 // ESIZE[cfg["dt"]]
    N, ldx = cfg["N"], cfg["ldx"]
    aligned = (cfg["off"] * ESIZE[cfg["dt"]]) % 16 == 0
    b = [f"colsum_{cfg['dt']}"]
    if not aligned:
        b.append("scalar_misaligned_base")
    elif ldx % vec_w:
        b.append("scalar_ldx")
    elif N % vec_w:
        b.append("vector+scalar_tail" if N > vec_w else "scalar_tail_only")
    else:
        b.append("vector_only")
    xb, ys, capped = cs_plan(cfg)
    b.append("ysplit_capped" if capped else ("row_slices>1" if ys > 1 else "one_row_slice"))
    b.append("accumulate" if cfg["accumulate"] else "overwrite")
    b.append("unscale" if cfg["unscale"] is not None else "no_unscale")
    return b


def cs_case(seed):
    rs = np.random.RandomState(7300 + seed)
    N = int(CS_N[seed % len(CS_N)])
    dt = [F32, BF16, F16][rs.randint(3)]
    ldx = int(rs.choice([N, N + 1, up(N, 8) + 8]))
    M = int(rs.choice([m for m in CS_M if m * ldx <= CS_MAX_ELEMS]))
    # off = 1: the base sliced by one column.  colsum_kernel tests the base address (`vec`) and then reads with ldf, one element per access
    return dict(fam="cs", seed=seed, N=N, M=M, dt=dt, ldx=ldx, off=int(rs.randint(3) == 0), accumulate=int(rs.randint(2)),
                unscale=[None, 0.25, 1.0 / 1024][rs.randint(3)])


CS_FIXED = [
    # enough rows x strips that the row slices are capped by the block budget: needs M * ceil(N / 128) > 2048 * 256
    dict(fam="cs", seed=9301, N=3072, M=40000, dt=F32, ldx=3072, off=0, accumulate=1, unscale=0.25),
    dict(fam="cs", seed=9302, N=30522, M=5000, dt=BF16, ldx=30528, off=0, accumulate=0, unscale=None),
    dict(fam="cs", seed=9303, N=30522, M=5000, dt=F16, ldx=30523, off=0, accumulate=1, unscale=1.0 / 1024),
]


def cs_cases():
    return [cs_case(s) for s in range(N_CS)] + CS_FIXED


CP_P = (1, 5, 8, 9, 130)
CP_N = (1, 63, 64, 65, 768, 3072)
N_CP = 30


def cp_branches(cfg):
    P, N, ld = cfg["P"], cfg["N"], cfg["ld"]
    xb = (N + 63) // 64
    ys = max(1, min((PARTIALS_BLOCKS + xb - 1) // xb, (P + 7) // 8))
    b = ["partials_one_slice" if ys == 1 else "partials_row_slices>1"]
    if P < 8:
        b.append("P<8")
    if P % 4:
        b.append("P%4")
    if N % 64:
        b.append("N%64")
    if ld > N:
        b.append("ld>N")
    b.append("unscale" if cfg["unscale"] is not None else "no_unscale")
    return b


def cp_case(seed):
    rs = np.random.RandomState(7350 + seed)
    P, N = int(CP_P[seed % len(CP_P)]), int(CP_N[(seed // len(CP_P)) % len(CP_N)])
    return dict(fam="cp", seed=seed, P=P, N=N, ld=N + int(rs.choice([0, 1, 8])), unscale=[None, 0.25][rs.randint(2)])


def cp_cases():
    return [cp_case(s) for s in range(N_CP)]


# =====================================================================================================================
# casts, add, dact, transpose
# =====================================================================================================================
CAST_PAIRS = ((F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, BF16), (BF16, F16), (F16, F16))
CAST2D_PAIRS = ((F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, F16))
CAST_N = (1, 2, 3, 4, 5, 1001)
CAST_BIG_N = ELEMWISE_SPAN + 4 + 3
CAST2D_ROWS = (1, 64)
CAST2D_BIG_ROWS = CAST2D_ROWS_PER_LAUNCH + 3
CAST2D_WIDE_LDD = CAST2D_COL_BLOCKS * 256 + 40
ADD_N = (4, 8, 1004, ELEMWISE_SPAN + 4096)
TRANSPOSE_SHAPES = ((768, 3072), (2304, 768), (65, 130), (1, 7))


def special_values():
    """f32 values every cast input carries: signed zeros, infinities, NaN, subnormals of each encoding, exact rounding ties of
    bf16 and f16 in both directions (to even = down, to even = up), and values around the f16 overflow threshold."""
    t8, t11 = 2.0 ** -8, 2.0 ** -11
    v = [0.0, -0.0, float("inf"), float("-inf"), float("nan"),
         1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126,                      # f32 / bf16 subnormals and the smallest normal
         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 3e-6, 2.0 ** -14, 6e-5,      # f16 subnormals, the tie to zero
         1 + t8, 1 + 3 * t8, -(1 + t8), -(1 + 3 * t8), 1 + t8 + 2.0 ** -20, 1 + t8 - 2.0 ** -20,      # bf16 ties / just off a tie
         1 + t11, 1 + 3 * t11, -(1 + t11), -(1 + 3 * t11), 1 + t11 + 2.0 ** -23,                     # f16 ties
         65504.0, 65519.0, 65520.0, -65520.0, 65536.0, 1e5, -7e4,                                    # around f16's largest value
         3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38, 1.0, -2.5, 0.333]     # FLT_MAX, largest bf16
    return torch.tensor(v, dtype=torch.float32)


def cast_input(n, src, seed):
    """CPU tensor [n] in the source encoding: random values with the special block at the front and again at the very end (the
    tail elements of n % 4), rotated by the seed so that short inputs see different specials."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n,), generator=g) * 3.0
    sp = special_values().roll(seed % 41)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n > 2 * sp.numel():
        x[n - sp.numel():] = sp.roll(3)
    return x.to(DT[src])


def cast_branches(cfg):
    n = cfg["n"]
    b = [f"cast_{cfg['src']}_to_{cfg['dst']}"]
    if n < 4:
        b.append("cast_tail_only")
    elif n & 3:
        b.append("cast_vector+tail")
    else:
        b.append("cast_vector_only")
    if n // 4 > ELEMWISE_BLOCKS * 256:
        b.append("cast_grid_stride")
    return b


def cast2d_branches(cfg):
    b = [f"cast2d_{cfg['src']}_to_{cfg['dst']}"]
    if cfg["rows"] > CAST2D_ROWS_PER_LAUNCH:
        b.append("cast2d_second_launch")
    if cfg["ldd"] > CAST2D_COL_BLOCKS * 256:
        b.append("cast2d_column_stride")
    if cfg["ldd"] > cfg["cols"]:
        b.append("cast2d_zero_fill")
    return b


def ew_branches(cfg):
    op = cfg["op"]
    if op == "cast":
        return cast_branches(cfg)
    if op == "cast2d":
        return cast2d_branches(cfg)
    if op in ("add", "dact"):
        name = f"add_{cfg['dt']}" if op == "add" else f"dact{cfg['mode']}_{cfg['dt']}"
        return [name] + ([f"{op}_grid_stride"] if cfg["n"] // 4 > ELEMWISE_BLOCKS * 256 else [])
    return [f"transpose_{cfg['dt']}"]


def ew_cases():
    cases, seed = [], 0

    def add(**kw):
        nonlocal seed
        cases.append(dict(fam="ew", seed=7400 + seed, **kw))
        seed += 1
    for src, dst in CAST_PAIRS:
        for n in CAST_N:
            add(op="cast", src=src, dst=dst, n=n)
    for src, dst in ((F32, BF16), (F32, F16), (F16, F32), (BF16, F16)):
        add(op="cast", src=src, dst=dst, n=CAST_BIG_N)
    for i, (src, dst) in enumerate(CAST2D_PAIRS):
        for j, rows in enumerate(CAST2D_ROWS):
            cols = (1, 5, 30, 48)[(i + j) % 4]
            for k, ldd in enumerate((cols, cols + 5, CAST2D_WIDE_LDD)):
                add(op="cast2d", src=src, dst=dst, rows=rows, cols=cols, lds=cols + (0, 3, 8)[(i + j + k) % 3], ldd=ldd)
    # the second launch chunk: rows beyond 65535; ldd < lds, so the two row pitches cannot stand in for each other
    for src, dst in ((F32, BF16), (F16, F32), (BF16, BF16)):
        add(op="cast2d", src=src, dst=dst, rows=CAST2D_BIG_ROWS, cols=48, lds=56, ldd=53)
    add(op="cast2d", src=F32, dst=F16, rows=CAST2D_BIG_ROWS, cols=5, lds=8, ldd=5)
    for dt in (F32, BF16, F16):
        for n in ADD_N[:3]:
            add(op="add", dt=dt, n=n)
            for mode in (0, 1, 2):
                add(op="dact", dt=dt, mode=mode, n=n)
    add(op="add", dt=F16, n=ADD_N[3])
    add(op="add", dt=F32, n=ADD_N[3])
    add(op="add", dt=BF16, n=ADD_N[3])
    add(op="dact", dt=BF16, mode=0, n=ADD_N[3])
    add(op="dact", dt=F16, mode=1, n=ADD_N[3])
    add(op="dact", dt=F32, mode=2, n=ADD_N[3])
    for dt in (F32, BF16, F16):
        for rows, cols in TRANSPOSE_SHAPES:
            add(op="transpose", dt=dt, rows=rows, cols=cols)
    return cases


def dgelu64(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


# =====================================================================================================================
# non-finite counter
# =====================================================================================================================
NF_N = (1, 2, 3, 5, 1024, 4097)
NF_BIG_N = ELEMWISE_SPAN + 7
NF_K = (0, 1, 2, 7)
# bit patterns planted as non-finite values: +inf, -inf, quiet NaN, negative NaN, signalling NaN with a payload, quiet NaN with a payload
NF_BITS = (0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fc12345, 0xff9abcde)
# finite values that must NOT count: +-FLT_MAX, subnormals, the smallest normal, signed zeros
NF_FINITE_BITS = (0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x00800000, 0x00000000, 0x80000000, 0x7f000000)


def nf_branches(cfg):
    n, pos = cfg["n"], nf_positions(cfg)
    b = ["count_planted" if cfg["k"] else "count_clean"]
    if n < 4:
        b.append("count_tail_only")
    if n & 3 and cfg["k"] and all(p >= n // 4 * 4 for p in pos):
        b.append("count_only_in_tail")
    if n & 3 and cfg["k"] and any(p >= n // 4 * 4 for p in pos):
        b.append("count_in_tail")
    if n // 4 > ELEMWISE_BLOCKS * 256:
        b.append("count_grid_stride")
    b.append("count_start=%d" % cfg["start"])
    return b


def nf_positions(cfg):
    """k distinct positions: always n - 1, position 0 when k > 1, the rest drawn"""
    n, k = cfg["n"], min(cfg["k"], cfg["n"])
    if k == 0:
        return []
    pos = {n - 1}
    if k > 1:
        pos.add(0)
    rs = np.random.RandomState(7550 + cfg["seed"])
    while len(pos) < k:
        pos.add(int(rs.randint(n)))
    return sorted(pos)


def nf_cases():
    cases = []
    for i, n in enumerate(NF_N + (NF_BIG_N,)):
        for j, k in enumerate(NF_K):
            cases.append(dict(fam="nf", seed=len(cases), n=n, k=min(k, n), start=(0, 5)[(i + j) % 2]))
    return cases


def nf_input(cfg):
    """CPU f32 [n]: finite data carrying +-FLT_MAX and subnormals, then the planted non-finite values.  -> (x, number planted)"""
    n = cfg["n"]
    g = torch.Generator().manual_seed(cfg["seed"])
    bits = (torch.randn((n,), generator=g) * 1e3).view(torch.int32).clone()
    fin = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in NF_FINITE_BITS], dtype=torch.int32).roll(cfg["seed"])
    m = min(n, fin.numel())
    bits[:m] = fin[:m]
    if n > 2 * fin.numel():
        bits[n - fin.numel():] = fin
    pos = nf_positions(cfg)
    for i, p in enumerate(pos):
        b = NF_BITS[(i + cfg["seed"]) % len(NF_BITS)]
        bits[p] = b - (1 << 32) if b >= (1 << 31) else b
    return bits.view(torch.float32), len(pos)


# =====================================================================================================================
# AdamW
# =====================================================================================================================
AW_N = (1, 2, 3, 5, 16, 4099)
AW_BIG_N = ADAMW_SPAN + 5
N_AW = 36


def aw_branches(cfg):
    n = cfg["n"]
    b = ["adamw_tail_only" if n < 4 else ("adamw_vector+tail" if n & 3 else "adamw_vector_only")]
    if n & 3 and cfg["shadows"] == "both":
        b.append("adamw_tail_both_shadows")
    if n // 4 > ADAMW_BLOCKS * 256:
        b.append("adamw_grid_stride")
    b.append("adamw_shadows_" + cfg["shadows"])
    b.append("adamw_state_" + cfg["state"])
    b.append("adamw_correct_bias=%d" % cfg["correct_bias"])
    b.append("adamw_grad_scale" if cfg["grad_scale"] != 1.0 else "adamw_no_grad_scale")
    return b


def aw_case(seed):
    rs = np.random.RandomState(7600 + seed)
    return dict(fam="aw", seed=seed, n=int(AW_N[seed % len(AW_N)]), correct_bias=int(rs.randint(2)), grad_scale=[1.0, 1.0 / 128][rs.randint(2)],
                shadows=("both", "bf16", "f16", "none")[(seed // len(AW_N)) % 4], state=("none", "none", "live", "skip")[rs.randint(4)],
                wd=[0.0, 0.01][rs.randint(2)])


AW_FIXED = [
    dict(fam="aw", seed=9601, n=AW_BIG_N, correct_bias=1, grad_scale=1.0 / 128, shadows="both", state="none", wd=0.01),
    dict(fam="aw", seed=9604, n=AW_BIG_N, correct_bias=0, grad_scale=1.0, shadows="bf16", state="live", wd=0.0),
    dict(fam="aw", seed=9605, n=AW_BIG_N - 1, correct_bias=1, grad_scale=1.0, shadows="f16", state="skip", wd=0.01),
    dict(fam="aw", seed=9602, n=4099, correct_bias=1, grad_scale=1.0, shadows="both", state="skip", wd=0.01),
    dict(fam="aw", seed=9603, n=3, correct_bias=0, grad_scale=1.0, shadows="both", state="live", wd=0.01),
]
AW_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6)


def aw_cases():
    return [aw_case(s) for s in range(N_AW)] + AW_FIXED


def hf_adamw_reference(p, grads, lr, b1, b2, eps, wd, correct_bias, grad_scale):
    """HF AdamW (<= 4.x) in fp64 over len(grads) steps from zero moments: the restatement oracle/ already has, fed with the f32-rounded
    hyper-parameters the kernel receives (1 - beta is exact in f32, so the f32 and the fp64 moment factors agree).
    -> per step (p, m, v) as fp64 clones."""
    from oracle.cxrbert_oracle import hf_adamw_step
    lr, b1, b2, eps = f32r(lr), f32r(b1), f32r(b2), f32r(eps)
    wd_eff = f32r(lr * f32r(wd)) / lr                      # the launcher hands the kernel the f32 product lr * wd
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, g in enumerate(grads, 1):
        hf_adamw_step(p, g.double() * f32r(grad_scale), m, v, t, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd_eff, correct_bias=bool(correct_bias))
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def aw_bounds(p_ref, g_abs_max, lr, steps):
    """f32 error bounds after `steps` steps, element-wise (p_ref fp64, g_abs_max = largest |g * grad_scale| seen per element).
    Each step is a handful of f32 operations without cancellation except in m: 4 roundings on m (relative to |g| at most, since
    |m| <= max|g|), 4 on v (relative to g^2), and about 16 on p, each relative to |p| or to the update, which is at most
    (1 - b1) / sqrt(1 - b2) * sqrt(steps) * lr < 6 lr for three steps (Cauchy-Schwarz on the moment sums), bias-corrected or not."""
    return (steps * 16 * U32 * (p_ref.abs() + 6.0 * lr), steps * 4 * U32 * g_abs_max, steps * 4 * U32 * g_abs_max ** 2)


# =====================================================================================================================
# dropout mask
# =====================================================================================================================
DM_N = (1, 2, 3, 65536, 2000001)
DM_P = (0.0, 0.1, 0.5)
DM_KEYS = (0x0123456789abcdef, 77)


def dm_cases():
    return [dict(fam="dm", seed=i, n=n, p=p) for i, (n, p) in enumerate((n, p) for n in DM_N for p in DM_P)]


def dm_branches(cfg):
    b = ["mask_p=%g" % cfg["p"], "mask_odd_n" if cfg["n"] & 1 else "mask_even_n"]
    if cfg["n"] > DROPMASK_BLOCKS * 256:
        b.append("mask_grid_stride")
    if cfg["n"] >= 65536:
        b.append("mask_statistics")
    return b


def dm_threshold(p):
    """mv_make_drop: an element is dropped when its 16-bit half of the pair's hash is below thr"""
    return 0 if p <= 0 else min(65535, int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))


HASH_MUL = (0x9E3779B1, 0x85EBCA6B)          # mv_hash32 (csrc/mv_common.h): the two multipliers, the three xor-shifts
HASH_SHIFT = (15, 13, 16)


def hash32(x, key):
    """mv_hash32(x, k0 = key & 0xffffffff, k1 = key >> 32) of csrc/mv_common.h for an array of 32-bit counters: uint64 arithmetic masked
    to 32 bits after every multiply -> uint64 array of values < 2^32.  The one restatement of the hash in the tests: the hidden-state
    dropout mask (dm_restated) and the MLM draws (tests/batch_cases.py) both come from here."""
    m = np.uint64(0xffffffff)
    x = np.asarray(x, dtype=np.uint64) & m
    k0, k1 = np.uint64(int(key) & 0xffffffff), np.uint64((int(key) >> 32) & 0xffffffff)
    x = ((x ^ k0) * np.uint64(HASH_MUL[0])) & m
    x ^= x >> np.uint64(HASH_SHIFT[0])
    x = ((x ^ k1) * np.uint64(HASH_MUL[1])) & m
    x ^= x >> np.uint64(HASH_SHIFT[1])
    x ^= x >> np.uint64(HASH_SHIFT[2])
    return x


def dm_restated(p, key, n):
    """The mask written out with numpy: one 32-bit hash per PAIR of elements (index >> 1), element i reads half i & 1."""
    thr = dm_threshold(p)
    i = np.arange(n, dtype=np.uint64)
    x = hash32(i >> np.uint64(1), key).astype(np.uint32)
    half = (x >> (np.uint32(16) * (i & np.uint64(1)).astype(np.uint32))) & np.uint32(0xffff)
    return (half >= thr).astype(np.uint8) if thr else np.ones(n, dtype=np.uint8)


# =====================================================================================================================
# census
# =====================================================================================================================
FAMILIES = {
    "ce": (ce_cases, ce_branches),
    "ln": (ln_cases, lambda c: ln_fwd_branches(c) + ln_bwd_branches(c)),
    "gs": (gs_cases, gs_branches),
    "cs": (cs_cases, cs_branches),
    "cp": (cp_cases, cp_branches),
    "ew": (ew_cases, ew_branches),
    "nf": (nf_cases, nf_branches),
    "aw": (aw_cases, aw_branches),
    "dm": (dm_cases, dm_branches),
}


def census(fam):
    """branch name -> number of cases of the family that reach it"""
    cases, branches = FAMILIES[fam]
    count = {}
    for c in cases():
        for b in branches(c):
            count[b] = count.get(b, 0) + 1
    return count
