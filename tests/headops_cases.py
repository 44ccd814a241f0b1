"""Case generators, dispatch predicates, fp64 references and error bounds of the sweep of the fine-tuning loss and optimizer kernels
(csrc/mv_lmloss.hip: mv_lm_loss_fwd / _select / _bwd; csrc/mv_vqa.hip: mv_bce_fwd_bwd, mv_rows_mul; csrc/mv_optim.hip:
mv_tensor_sqnorms, mv_bertadam_step, mv_bce_multilabel).

Plain module: nothing here touches the GPU or the HIP library.  tests/test_headops_sweep_gpu.py runs the cases on the kernels, and
tests/test_headops_cases_cpu.py counts which branch every case takes, reads the caps below out of the .hip sources, and shows that
the bounds let an honest f32 restatement through and catch each planted defect.

* a cfg dict holds everything a case is made of; the tensors come from cfg["seed"] alone, so a printed cfg reproduces the case;
* `*_branch(cfg)` restates the launcher's conditions and names the branches and value classes a case reaches;
* `*_inputs(cfg)` builds host tensors (numpy); `*_reference(cfg, inp)` the fp64 result with ONE BOUND PER OUTPUT ELEMENT;
* `*_restated(cfg, inp, defect)` is the kernel written again in numpy float32 with another summation order, with switches that
  plant one defect each; `*_judge(cfg, inp, ref, out)` is the one judgement both test files apply (-> ok, worst error / bound, what).

Bounds.  Every bound is a sum of unit roundoffs times the magnitudes of the terms an element is formed from (cancelling terms by
their absolute values), times SLACK for the second-order terms, plus FLOOR (below the smallest normal f32 the relative error model
does not hold: expf underflows).  A 16-bit store adds half an ulp of the encoding (HALF_ULP_REL; f16 adds its subnormal quantum).
Sums use the n-term bound rowops_cases.sum_bound.  The device math functions enter through the constants below.
"""
import math

import numpy as np
import torch

from rowops_cases import BF16, DT, ESIZE, F16, F16_SUBNORMAL_HALF_ULP, F32, U16, U32, f32r, sum_bound, up  # noqa: F401

# ---- accuracy of the device math functions, in ulps.  The HIP math documentation is not at hand, so these are ASSUMED: 2 ulp for the
# f32 transcendentals, 0.5 ulp (correctly rounded) for sqrtf and f32 division, 1 ulp for log in double.
ULP_EXPF = 2.0
ULP_LOG1PF = 2.0
ULP_SQRTF = 0.5
ULP_DIV = 0.5
ULP_LOG64 = 1.0
ULP32 = 2.0 * U32                                  # one f32 ulp relative to the value, at most
E_EXP, E_L1P, E_SQRT, E_DIV = ULP_EXPF * ULP32, ULP_LOG1PF * ULP32, ULP_SQRTF * ULP32, ULP_DIV * ULP32
U64 = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -10
FLOOR = 2.0 ** -120
HALF_ULP_REL = {F32: 0.0, BF16: 2.0 * U16[BF16], F16: U16[F16]}      # bf16 keeps 8 significant bits: half an ulp is up to 2^-8 |v|
GUARD = 16                                         # elements around every output buffer (whole 16-byte vectors in every encoding)
NAN = float("nan")

# ---- caps of the kernels (tests/test_headops_cases_cpu.py reads the same numbers out of the .hip sources) ---------------------------
BLOCK = 256                    # lm_*, bce_kernel, bertadam, sq_chunk: threads per block
WAVE = 64                      # bce_ml_kernel: one wave per row; rows_mul: one wave per row, four per block
VEC_STRIDE = 1024              # columns one trip of a 256-thread x 4-element vector loop covers
ROWS_MUL_STRIDE = 256          # 64 lanes x 4 columns
SELECT_MAX_B = 2048
SELECT_LDS_PER_SAMPLE = 24
OPTIM_CHUNK = 4096
SCHEDULES = ("warmup_linear", "warmup_constant", "warmup_cosine")


def within(got, ref, bound):
    """numpy: -> (ok, worst error / bound); a non-finite difference is never ok"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.size == 0:
        return True, 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - ref)
        r = float(np.max(err / (bound + 1e-300)))
    ok = bool(np.all(np.isfinite(err))) and r <= 1.0
    return ok, (r if ok or math.isfinite(r) else float("inf"))


def store_bound(ref, b32, enc):
    """bound of a value computed in f32 within b32 and stored in `enc`"""
    b = b32 * SLACK + FLOOR
    if enc != F32:
        b = b + HALF_ULP_REL[enc] * (np.abs(ref) + b)
        if enc == F16:
            b = b + F16_SUBNORMAL_HALF_ULP
    return b


def to_enc(x, enc):
    """numpy f32/f64 -> torch tensor of the encoding (through f32: one rounding for values that are f32 already)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DT[enc])


def as64(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def case_id(cfg):
    skip = ("fam", "seed")
    def s(v):
        return "x".join(str(i) for i in v) if isinstance(v, (tuple, list)) else str(v)
    return "%s%d-" % (cfg["fam"], cfg["seed"]) + "-".join("%s%s" % (k, s(v)) for k, v in cfg.items() if k not in skip)


class Verdict:
    """collects the checks of one case: exact ones and bounded ones"""

    def __init__(self):
        self.ok, self.worst, self.what = True, 0.0, []

    def exact(self, name, cond):
        if not bool(cond):
            self.ok = False
            self.what.append(name + ": exact check failed")

    def bounded(self, name, got, ref, bound):
        ok, r = within(got, ref, bound)
        self.worst = max(self.worst, r)
        if not ok:
            self.ok = False
            self.what.append("%s: error / bound = %.3g" % (name, r))

    def result(self):
        return self.ok, self.worst, "; ".join(self.what)


def _sigmoid_parts(z):
    """fp64: e = exp(-|z|), sigmoid(z), log1p(e)"""
    e = np.exp(-np.abs(z))
    sg = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return e, sg, np.log1p(e)


D_SIG = E_EXP + U32 + E_DIV                        # relative error of the kernels' sigmoid: expf, 1 + e, the division


def _sigmoid32(z):
    e = np.exp(-np.abs(z)).astype(np.float32)
    one = np.float32(1.0)
    return e, np.where(z >= 0, one / (one + e), e / (one + e)).astype(np.float32)


# =====================================================================================================================
# rmul: mv_rows_mul (bit-exact)
# =====================================================================================================================
RMUL_H = (4, 128, 252, 256, 260, 768, 1024)
RMUL_R = (1, 3, 4, 5, 9)
RMUL_NEG = ("none", "a", "b", "both")
N_RMUL = 84


def rmul_case(i):
    return dict(fam="rmul", seed=100 + i, H=RMUL_H[i % 7], R=RMUL_R[(i // 3) % 5], dt=(F32, BF16, F16)[(i // 7) % 3], pad=(i // 21) % 2 * 8,
                same=bool((i // 2) % 2), neg=RMUL_NEG[(i // 7 + i) % 4])


def rmul_cases():
    return [rmul_case(i) for i in range(N_RMUL)]


def rmul_branch(cfg):
    H, R = cfg["H"], cfg["R"]
    b = ["rmul_" + cfg["dt"], "rmul_one_trip" if H <= ROWS_MUL_STRIDE else "rmul_trips>1"]
    b.append("rmul_partial_last_trip" if H % ROWS_MUL_STRIDE else "rmul_whole_trips")
    b.append("rmul_ld>H" if cfg["pad"] else "rmul_ld==H")
    b.append("rmul_same_buffer" if cfg["same"] else "rmul_two_buffers")
    b.append("rmul_neg_" + cfg["neg"])
    b.append("rmul_idle_waves" if R % 4 else "rmul_full_blocks")
    b.append("rmul_blocks>1" if R > 4 else "rmul_one_block")
    return b


def rmul_inputs(cfg):
    rs = np.random.RandomState(cfg["seed"])
    H, R, ld, NA = cfg["H"], cfg["R"], cfg["H"] + cfg["pad"], 7

    def buf():
        x = (np.exp2(rs.uniform(-3, 3, (NA, ld))) * rs.choice([-1.0, 1.0], (NA, ld))).astype(np.float32)
        x[:, H:] = NAN
        return to_enc(x, cfg["dt"])
    a = buf()
    b = a if cfg["same"] else buf()
    ra, rb = rs.randint(0, NA, R).astype(np.int32), rs.randint(0, NA, R).astype(np.int32)
    hit = rs.randint(0, R)
    neg = cfg["neg"]
    if neg in ("a", "both"):
        ra[hit] = -1
    if neg in ("b", "both"):
        rb[hit if neg == "b" or R == 1 else (hit + 1) % R] = -3
    return dict(a=a, b=b, ra=torch.from_numpy(ra), rb=torch.from_numpy(rb), ld=ld)


def rmul_reference(cfg, inp):
    """the whole [R, ld] output as it has to look: columns < H the rounded product (or zeros), guard columns NaN as filled"""
    H, R, ld = cfg["H"], cfg["R"], inp["ld"]
    ra, rb = inp["ra"].numpy(), inp["rb"].numpy()
    a, b = as64(inp["a"]), as64(inp["b"])
    out = np.full((R, ld), NAN)
    for i in range(R):
        out[i, :H] = a[ra[i], :H] * b[rb[i], :H] if ra[i] >= 0 and rb[i] >= 0 else 0.0
    # the fp64 product is exact; for the 16-bit types it is exact in f32 too, so .float() rounds nothing there
    return dict(out=torch.from_numpy(out).float().to(DT[cfg["dt"]]))


def rmul_restated(cfg, inp, defect=None):
    H, R, ld = cfg["H"], cfg["R"], inp["ld"]
    ra, rb = inp["ra"].numpy(), inp["rb"].numpy()
    a, b = inp["a"].float().numpy(), inp["b"].float().numpy()
    out = torch.full((R, ld), NAN, dtype=DT[cfg["dt"]])
    hi = min(H, ROWS_MUL_STRIDE) if defect == "cols_ge_256_skipped" else H
    for i in range(R):
        dead = ra[i] < 0 or (rb[i] < 0 and defect != "neg_b_ignored")
        v = np.zeros(hi, np.float32) if dead else a[ra[i], :hi] * b[max(rb[i], 0), :hi]
        out[i, :hi] = to_enc(v, cfg["dt"])
    return dict(out=out)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def rmul_judge(cfg, inp, ref, out):
    v, H = Verdict(), cfg["H"]
    got = out["out"].cpu()
    v.exact("out", got.dtype == ref["out"].dtype and torch.equal(bits(got[:, :H]), bits(ref["out"][:, :H])))
    v.exact("guard columns H..ld-1 still hold their NaN", bool(torch.isnan(got[:, H:].float()).all()))
    v.exact("guards", out.get("guards_ok", True))
    return v.result()


# =====================================================================================================================
# bceml: mv_bce_multilabel
# =====================================================================================================================
BCEML_C = (1, 14, 63, 64, 65, 130)
BCEML_R = (1, 37, 300)
BCEML_PW = ("none", "ones", "drawn", "one50")
BCEML_ABSENT = (None, "loss", "dgrad", "probs", "counters", "target")
N_BCEML = 72


def bceml_case(i):
    C = BCEML_C[i % 6]
    return dict(fam="bceml", seed=200 + i, C=C, R=BCEML_R[(i // 6) % 3], pw=BCEML_PW[(i // 2) % 4], ddt=(F32, BF16, F16)[(i // 6 + i) % 3],
                ld=C + (0, 3)[(i // 3) % 2], ldd=C + (0, 6)[(i // 4) % 2], absent=BCEML_ABSENT[(i // 6 + i // 18) % 6], gs=("host", "dev")[i % 2],
                ls=bool((i // 5) % 2), pattern=("gauss", "edges", "sat")[(i // 9 + i) % 3])


def bceml_cases():
    return [bceml_case(i) for i in range(N_BCEML)]


def bceml_branch(cfg):
    C = cfg["C"]
    b = ["bceml_C<64" if C < WAVE else "bceml_C==64" if C == WAVE else "bceml_second_trip", "bceml_pw_" + cfg["pw"]]
    b.append("bceml_inference" if cfg["absent"] == "target" else "bceml_no_" + cfg["absent"] if cfg["absent"] else "bceml_all_outputs")
    if cfg["absent"] not in ("target", "dgrad"):
        b += ["bceml_d_" + cfg["ddt"], "bceml_ldd>C" if cfg["ldd"] > C else "bceml_ldd==C", "bceml_gs_" + cfg["gs"],
              "bceml_ls_given" if cfg["ls"] else "bceml_ls_null"]
    b += ["bceml_ld>C" if cfg["ld"] > C else "bceml_ld==C", "bceml_" + cfg["pattern"], "bceml_two_calls"]
    return b


def bceml_has(cfg, name):
    """is the optional output `name` passed?"""
    return cfg["absent"] != name and (cfg["absent"] != "target" or name in ("probs", "arg_infer"))


def bceml_inputs(cfg):
    """two draws (the two calls accumulate into one loss and one set of counters)"""
    rs = np.random.RandomState(cfg["seed"])
    C, R = cfg["C"], cfg["R"]
    calls = []
    for _ in range(2):
        z = np.full((R, cfg["ld"]), NAN, np.float32)
        z[:, :C] = rs.randn(R, C) * 3.0
        y = (rs.rand(R, C) < 0.3).astype(np.float32)
        if cfg["pattern"] == "edges":                      # z == +-0 is a negative prediction, y == 0.5 a negative target
            z[:, :C][rs.rand(R, C) < 0.25] = 0.0
            z[:, :C][rs.rand(R, C) < 0.1] = -0.0
            y[rs.rand(R, C) < 0.25] = 0.5
            z[0, 0], y[0, 0] = 0.0, 1.0
            z[0, C - 1], y[0, C - 1] = 0.0, 0.5
        if cfg["pattern"] == "sat":
            z[:, :C][rs.rand(R, C) < 0.3] = 80.0
            z[:, :C][rs.rand(R, C) < 0.3] = -80.0
        calls.append((z, y))
    pw = {"none": None, "ones": np.ones(C, np.float32), "drawn": rs.uniform(0.2, 5.0, C).astype(np.float32)}.get(cfg["pw"])
    if cfg["pw"] == "one50":
        pw = rs.uniform(0.2, 5.0, C).astype(np.float32)
        pw[rs.randint(0, C)] = 50.0
    return dict(calls=calls, pw=pw, gs=f32r(1.0 / R), lsv=1024.0 if cfg["ls"] else None, loss0=3.25, counters0=5.0)


def _gs32(inp):
    """the f32 product the kernels form: grad scale x loss scale"""
    return np.float32(inp["gs"]) * np.float32(inp["lsv"]) if inp["lsv"] is not None else np.float32(inp["gs"])


def bceml_reference(cfg, inp):
    C = cfg["C"]
    w = np.ones(C) if inp["pw"] is None else inp["pw"].astype(np.float64)
    gs = float(inp["gs"]) * (inp["lsv"] or 1.0)
    ref = dict(calls=[])
    tot, tot_abs, tot_err = inp["loss0"], abs(inp["loss0"]), 0.0
    cnt = np.full((3, C), inp["counters0"])
    for z32, y32 in inp["calls"]:
        z, y = z32[:, :C].astype(np.float64), y32.astype(np.float64)
        e, sg, l = _sigmoid_parts(z)
        k = w * y + 1.0 - y
        r = sg * k - w * y
        dk = U32 * (np.abs(w * y) + np.abs(w * y + 1.0) + np.abs(k))
        dr = sg * dk + np.abs(k) * sg * (D_SIG + U32) + U32 * np.abs(w * y) + U32 * np.abs(r)
        g_b = abs(gs) * dr + 2 * U32 * np.abs(r * gs)
        a, q, s = 1.0 - y, 1.0 + (w - 1.0) * y, np.maximum(-z, 0.0) + l
        dq = U32 * (2 * np.abs((w - 1.0) * y) + np.abs(q))
        ds = l * (E_EXP + E_L1P) + U32 * s
        el = a * z + q * s
        d_el = 2 * U32 * np.abs(a * z) + s * dq + np.abs(q) * ds + U32 * np.abs(q * s) + U32 * (np.abs(a * z) + np.abs(q * s))
        tot, tot_abs, tot_err = tot + el.sum(), tot_abs + np.abs(el).sum(), tot_err + d_el.sum()
        pos, pred = y > 0.5, z > 0
        cnt = cnt + np.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)])
        ref["calls"].append(dict(grad=r * gs, grad_b=store_bound(r * gs, g_b, cfg["ddt"]), probs=sg, probs_b=store_bound(sg, sg * D_SIG, F32)))
    # a row's C terms in f32, then one atomic per row and call onto the running total
    ref.update(loss=tot, loss_b=(tot_err + sum_bound(C + 2 * cfg["R"] + 1, tot_abs)) * SLACK, counters=cnt)
    return ref


def bceml_restated(cfg, inp, defect=None):
    """-> the outputs in the form the runner collects them: loss [1], counters [3, C], per call dgrad [R, ldd] (NaN beyond) / probs"""
    C, R, ldd = cfg["C"], cfg["R"], cfg["ldd"]
    hi = min(C, WAVE) if defect == "cols_ge_64_skipped" else C
    one = np.float32(1.0)
    w = np.ones(C, np.float32) if inp["pw"] is None else inp["pw"]
    gs = _gs32(inp)
    loss, cnt, calls = np.float32(inp["loss0"]), np.full((3, C), inp["counters0"], np.float32), []
    for z32, y in inp["calls"]:
        z, yy, ww = z32[:, :hi], y[:, :hi], w[:hi]
        e, sg = _sigmoid32(z)
        l = np.log1p(e).astype(np.float32)
        if defect == "pos_weight_on_negative":
            el = yy * (np.maximum(-z, 0) + l) + ww * (one - yy) * (np.maximum(z, 0) + l)
        else:
            el = (one - yy) * z + (one + (ww - one) * yy) * (np.maximum(-z, 0) + l)
        loss = np.float32(loss + np.sum(el.astype(np.float32)[:, ::-1], dtype=np.float32))
        d = np.full((R, ldd), NAN, np.float32)
        d[:, :hi] = (sg * (ww * yy + one - yy) - ww * yy) * gs
        d[:, C:] = 0.0
        p = np.full((R, C), NAN, np.float32)
        p[:, :hi] = sg
        pos, pred = yy > 0.5, (z >= 0 if defect == "pred_at_z>=0" else z > 0)
        cnt[:, :hi] += np.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)]).astype(np.float32)
        calls.append(dict(dgrad=to_enc(d, cfg["ddt"]) if bceml_has(cfg, "dgrad") else None, probs=p if bceml_has(cfg, "probs") else None))
    return dict(loss=np.array([loss]) if bceml_has(cfg, "loss") else None, counters=cnt if bceml_has(cfg, "counters") else None, calls=calls)


def _grad_checks(v, name, got, ref, bound, width):
    """a gradient buffer [R, ldd]: columns < width under the bound, the rest exactly zero"""
    g = as64(got)
    v.bounded(name, g[:, :width], ref, bound)
    v.exact(name + " pad columns zero", np.all(g[:, width:] == 0.0))


def bceml_judge(cfg, inp, ref, out):
    v, C = Verdict(), cfg["C"]
    if bceml_has(cfg, "loss"):
        v.bounded("loss", as64(out["loss"]).reshape(-1)[:1], [ref["loss"]], [ref["loss_b"]])
    if bceml_has(cfg, "counters"):
        v.exact("counters", np.array_equal(as64(out["counters"]).reshape(3, C), ref["counters"]))
    for k, (o, r) in enumerate(zip(out["calls"], ref["calls"])):
        if bceml_has(cfg, "dgrad"):
            _grad_checks(v, "dgrad[%d]" % k, o["dgrad"], r["grad"], r["grad_b"], C)
        if bceml_has(cfg, "probs"):
            v.bounded("probs[%d]" % k, as64(o["probs"]).reshape(-1, C), r["probs"], r["probs_b"])
    return v.result()


# =====================================================================================================================
# bce: mv_bce_fwd_bwd
# =====================================================================================================================
BCE_A = (1, 2, 3, 255, 256, 257, 458, 513, 1025)
BCE_R = (1, 5, 37)
BCE_DDT = (None, F32, BF16, F16)
BCE_ABSENT = (None, "stats", "arg_train", "arg_infer", "target")
BCE_TIES = ("none", "adjacent", "wave64", "trip256", "col0", "allequal", "last")
BCE_PATTERNS = ("gauss", "sat", "zero", "neg")
N_BCE = 108


def _bce_tie(A, want):
    """the tie placement a row of A columns can hold"""
    need = {"none": 1, "adjacent": 3, "wave64": 67, "trip256": 258, "col0": 2, "allequal": 1, "last": 2}
    return want if A >= need[want] else ("allequal" if want != "none" else "none")


def bce_case(i):
    A = BCE_A[i % 9]
    return dict(fam="bce", seed=300 + i, A=A, R=BCE_R[(i // 9 + i) % 3], ld=A + (0, 1, 6)[(i // 9) % 3], ldd=A + (0, 6)[(i // 2) % 2],
                ddt=BCE_DDT[(i // 9) % 4], absent=BCE_ABSENT[(i // 4) % 5], ans=bool((i // 7) % 2), gs=("host", "dev")[i % 2], ls=bool((i // 5) % 2),
                tie=_bce_tie(A, BCE_TIES[(i // 9 + 2 * i) % 7]), pattern=BCE_PATTERNS[(i // 27 + i) % 4], init=bool(i % 3))


def bce_cases():
    return [bce_case(i) for i in range(N_BCE)]


def bce_has(cfg, name):
    if cfg["absent"] == "target":
        return name == "arg_infer"
    if name == "dgrad":
        return cfg["ddt"] is not None
    return cfg["absent"] != name


def bce_branch(cfg):
    A = cfg["A"]
    b = ["bce_A<=256" if A <= BLOCK else "bce_second_trip", "bce_idle_threads" if A < BLOCK else "bce_no_idle_thread"]
    if A == 1:
        b.append("bce_A==1_infer_fallback")
    b.append("bce_inference" if cfg["absent"] == "target" else "bce_no_" + cfg["absent"] if cfg["absent"] else "bce_all_outputs")
    if bce_has(cfg, "dgrad"):
        b += ["bce_d_" + cfg["ddt"], "bce_ldd>A" if cfg["ldd"] > A else "bce_ldd==A", "bce_gs_" + cfg["gs"], "bce_ls_given" if cfg["ls"] else "bce_ls_null"]
    elif cfg["absent"] != "target":
        b.append("bce_d_none")
    if cfg["absent"] != "target" and bce_has(cfg, "stats"):
        b.append("bce_ans_type_0/1/2" if cfg["ans"] else "bce_ans_type_absent")
    b += ["bce_ld-A=%d" % (cfg["ld"] - A), "bce_tie_" + cfg["tie"], "bce_" + cfg["pattern"]]
    return b


def bce_inputs(cfg):
    rs = np.random.RandomState(cfg["seed"])
    A, R, pat = cfg["A"], cfg["R"], cfg["pattern"]
    z = np.full((R, cfg["ld"]), NAN, np.float32)
    zz = (rs.randn(R, A) * 3.0).astype(np.float32)
    y = rs.choice([0.0, 0.0, 0.0, 0.3, 0.6, 0.9, 1.0], (R, A)).astype(np.float32)
    if pat == "sat":
        zz[rs.rand(R, A) < 0.3] = 80.0
        zz[rs.rand(R, A) < 0.3] = -80.0
    if pat == "zero":
        zz[rs.rand(R, A) < 0.2] = 0.0
        zz[rs.rand(R, A) < 0.2] = -0.0
    if pat == "neg":                                       # every term of the loss is log1p(exp(z)) alone: the stable split matters
        zz = rs.uniform(-14.0, -10.0, (R, A)).astype(np.float32)
        y[:] = 0.0
    top = np.float32(np.abs(zz).max() + 1.0) if pat != "neg" else np.float32(-9.0)
    for r in range(R):
        t = cfg["tie"]
        if t == "adjacent":
            c = rs.randint(1, A - 1)
            zz[r, [c, c + 1]] = top
        elif t == "wave64":
            c = rs.randint(1, min(A - 65, 191) + 1)
            zz[r, [c, c + 64]] = top
        elif t == "trip256":
            c = rs.randint(1, A - 256)
            zz[r, [c, c + 256]] = top
        elif t == "col0":
            zz[r, 0] = top
        elif t == "allequal":
            zz[r, :] = np.float32(0.75) if pat != "neg" else np.float32(-11.0)
        elif t == "last":
            zz[r, A - 1] = top
    z[:, :A] = zz
    ans = rs.randint(0, 3, R).astype(np.int32) if cfg["ans"] else None
    return dict(z=z, y=y, ans=ans, gs=f32r(0.5 / R), lsv=512.0 if cfg["ls"] else None,
                stats0=np.arange(1, 7, dtype=np.float32) if cfg["init"] and pat != "neg" else np.zeros(6, np.float32))


def bce_reference(cfg, inp):
    A, R = cfg["A"], cfg["R"]
    z32 = inp["z"][:, :A]
    z, y = z32.astype(np.float64), inp["y"].astype(np.float64)
    at = np.argmax(z32, axis=1)                            # the first maximum
    ai = 1 + np.argmax(z32[:, 1:], axis=1) if A > 1 else np.zeros(R, np.int64)
    e, sg, l = _sigmoid_parts(z)
    gs = float(inp["gs"]) * (inp["lsv"] or 1.0)
    r = sg - y
    g_b = abs(gs) * (sg * D_SIG + U32 * np.abs(r)) + 2 * U32 * np.abs(r * gs)
    el = np.maximum(z, 0.0) - z * y + l
    d_el = U32 * (2 * np.abs(z * y) + np.maximum(z, 0.0) + np.abs(el)) + l * (E_EXP + E_L1P)
    score = y[np.arange(R), at]
    s0 = inp["stats0"].astype(np.float64)
    ty = inp["ans"] if inp["ans"] is not None else np.full(R, -1)
    stats = s0 + np.array([score.sum(), el.sum(), score[ty == 0].sum(), (ty == 0).sum(), score[ty == 1].sum(), (ty == 1).sum()])
    sabs = np.abs(s0) + np.array([score.sum(), np.abs(el).sum(), score[ty == 0].sum(), (ty == 0).sum(), score[ty == 1].sum(), (ty == 1).sum()])
    sb = sum_bound(R + 1, sabs)
    sb[1] += d_el.sum() + sum_bound(A, np.abs(el).sum())   # the row's A terms in f32 before the atomic
    sb[[3, 5]] = 0.0                                       # integer-valued f32 counts: exact
    return dict(at=at, ai=ai, grad=r * gs, grad_b=store_bound(r * gs, g_b, cfg["ddt"] or F32), stats=stats, stats_b=sb * SLACK + FLOOR * (sb > 0))


def _argmax_by_waves(zrow, cross_wave_higher=False):
    """the first maximum found the kernel's way: per wave (columns c with (c % 256) // 64 == w), then across the four waves"""
    best, col = -np.inf, 0x7fffffff
    for w in range(4):
        cols = np.nonzero((np.arange(zrow.size) % BLOCK) // WAVE == w)[0]
        if cols.size == 0 or not np.any(zrow[cols] > -np.inf):
            continue
        c = cols[np.argmax(zrow[cols])]
        if zrow[c] > best or (zrow[c] == best and ((c > col) if cross_wave_higher else (c < col))):
            best, col = zrow[c], c
    return col


def bce_restated(cfg, inp, defect=None):
    A, R, ldd = cfg["A"], cfg["R"], cfg["ldd"]
    hi = min(A, BLOCK) if defect == "cols_ge_256_skipped" else A
    z, y = inp["z"][:, :hi], inp["y"][:, :hi]
    one = np.float32(1.0)
    at, ai = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for r in range(R):
        at[r] = _argmax_by_waves(z[r], defect == "cross_wave_tie_higher")
        if defect == "infer_may_return_0":
            ai[r] = at[r]
        else:
            zi = z[r].copy()
            zi[0] = -np.inf
            ai[r] = _argmax_by_waves(zi, defect == "cross_wave_tie_higher")
        if ai[r] >= A:
            ai[r] = 1 if A > 1 else 0
    out = dict(arg_train=at if bce_has(cfg, "arg_train") else None, arg_infer=ai if bce_has(cfg, "arg_infer") else None, stats=None, dgrad=None)
    if cfg["absent"] == "target":
        return out
    e, sg = _sigmoid32(z)
    if defect == "unstable_loss":
        el = np.log(one + np.exp(z).astype(np.float32)).astype(np.float32) - z * y
    else:
        el = np.maximum(z, 0) - z * y + np.log1p(e).astype(np.float32)
    if bce_has(cfg, "dgrad"):
        d = np.full((R, ldd), NAN, np.float32)
        d[:, :hi] = (sg - y) * _gs32(inp)
        d[:, A:] = 0.0
        out["dgrad"] = to_enc(d, cfg["ddt"])
    if bce_has(cfg, "stats"):
        st = inp["stats0"].copy()
        for r in reversed(range(R)):
            score = inp["y"][r, at[r]]
            st[0] += score
            st[1] += np.sum(el[r].astype(np.float32), dtype=np.float32)
            ty = inp["ans"][r] if inp["ans"] is not None else -1
            if ty in (0, 1):
                st[2 + 2 * ty] += score
                st[3 + 2 * ty] += one
        out["stats"] = st
    return out


def bce_judge(cfg, inp, ref, out):
    v = Verdict()
    if bce_has(cfg, "arg_train"):
        v.exact("arg_train", np.array_equal(as64(out["arg_train"]), ref["at"]))
    if bce_has(cfg, "arg_infer"):
        v.exact("arg_infer", np.array_equal(as64(out["arg_infer"]), ref["ai"]))
    if bce_has(cfg, "dgrad"):
        _grad_checks(v, "dgrad", out["dgrad"], ref["grad"], ref["grad_b"], cfg["A"])
    if bce_has(cfg, "stats"):
        v.bounded("stats", as64(out["stats"]).reshape(-1), ref["stats"], ref["stats_b"])
    return v.result()


# =====================================================================================================================
# the report objective: shared pieces of lmf / lmb / lmchain
# =====================================================================================================================
LM_V = (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 4099, 30522)
LM_SMOOTH = (0.0, 0.1, 1.0)
WORKLOAD_V, WORKLOAD_LD, WORKLOAD_ROWS = 30522, 30528, 8


def lm_const(ls, V):
    """lm_const() of mv_lmloss.hip: (smooth, conf in double, sval f32, qsum f32)"""
    smooth = ls > 0.0
    conf = 1.0 - ls
    sval = f32r(ls / (V - 2)) if smooth else 0.0
    qsum = f32r(conf + (V - 2) * sval) if smooth else 1.0
    return smooth, conf, sval, qsum


def lm_row_loss(zrow, labels, ls):
    """fp64 loss of every label on one row (V columns, f32 values) -> (losses, M, S, lse, logp).  With smoothing this is
    sum_c q (log q - logp) of the target row q = sval everywhere, 0 in column 0, conf in the label's column, written per label;
    tests/test_headops_cases_cpu.py holds it against report_finetune_cases.slot_loss."""
    z = zrow.astype(np.float64)
    V = z.size
    M = z.max()
    S = math.fsum(np.exp(z - M))
    lse = M + math.log(S)
    logp = z - lse
    smooth, conf, sval, _ = lm_const(ls, V)
    labels = np.asarray(labels, np.int64)
    if not smooth:
        return -logp[labels], M, S, lse, logp
    rest = math.fsum(logp[1:])
    xlx = (conf * math.log(conf) if conf > 0 else 0.0) + (V - 2) * sval * math.log(sval)
    out = xlx - conf * logp[labels] - sval * (rest - logp[labels])
    return np.where(labels == 0, 0.0, out), M, S, lse, logp


def lm_thread_rises(zrow, vec):
    """the largest number of times one thread's running maximum rises in lm_row_pass (the thread's columns in its order)"""
    V = zrow.size
    span = VEC_STRIDE if vec else BLOCK
    zp = np.full(up(V, span), -np.inf, np.float32)
    zp[:V] = zrow
    seq = zp.reshape(-1, BLOCK, 4).transpose(1, 0, 2).reshape(BLOCK, -1) if vec else zp.reshape(-1, BLOCK).T
    run = np.maximum.accumulate(seq, axis=1)
    rises = 1 + (seq[:, 1:] > run[:, :-1]).sum(1)
    return int(rises.max())


def lm_sum_relerr(zrow, vec):
    """bound of |S_kernel - S| / S for the online sum: every term carries its own expf (E_EXP, argument rounded: U32 (m - x)) and one
    more per rescale it lives through -- the rises of its thread, six shuffle merges, three wave merges -- whose exponents sum to at
    most m - x again; then the rounding of the double sum to f32"""
    z = zrow.astype(np.float64)
    fin = np.isfinite(z)
    d = np.where(fin, z.max() - z, 0.0)
    t = np.where(fin, np.exp(-d), 0.0)
    k = lm_thread_rises(zrow, vec) + 9
    return float(np.sum(t * ((1 + k) * E_EXP + 2 * U32 * d)) / np.sum(t)) + U32 + zrow.size * U64


def _lm_row(rs, V, pattern, vec):
    """one f32 row of V columns -> (row, pattern it could hold)"""
    z = (rs.randn(V) * 3.0).astype(np.float32)
    wave_gap, trip_gap = (256, 1024) if vec else (64, 256)
    top = np.float32(np.abs(z).max() + 2.0)

    def dup(gap):
        c = rs.randint(0, V - gap)
        z[[c, c + gap]] = top
    if pattern == "sat" and V >= 2:
        z[:] = -80.0
        z[rs.rand(V) < 0.4] = 80.0
        z[rs.randint(0, V)] = 80.0
    elif pattern == "equal":
        z[:] = 1.5
    elif pattern == "asc" and V >= 2:
        z = (-8.0 + 16.0 * np.arange(V) / V).astype(np.float32)
    elif pattern == "desc" and V >= 2:
        z = (8.0 - 16.0 * np.arange(V) / V).astype(np.float32)
    elif pattern == "outlier":
        z[rs.randint(0, V)] = 60.0
    elif pattern == "dup_trip" and V > trip_gap:
        dup(trip_gap)
    elif pattern == "dup_lane" and V > 4:
        dup(4)
    elif pattern == "dup_wave" and V > wave_gap:
        dup(wave_gap)
    elif pattern == "max0":
        z[0] = top
    elif pattern == "maxlast":
        z[V - 1] = top
    elif pattern != "neginf":
        pattern = "gauss"
    return z, pattern


def _lm_labels(rs, V, n, avoid=()):
    """n labels: the specials first (0, 1, V-1, inside the last partial vector, 1023 / 1024, one >= 1024), then drawn ones"""
    sp = [0, 1, V - 1, max(V - 2, 0), 4 * ((V - 1) // 4), 1023, 1024, 1024 + (V - 1024) // 2]
    sp = [c for c in sp if 0 <= c < V and c not in avoid]
    rs.shuffle(sp)
    lab = (sp + [int(c) for c in rs.randint(0, V, max(n - len(sp), 0)) if c not in avoid] + [0] * n)[:n]
    return np.array(lab, np.int32)


# =====================================================================================================================
# lmf: mv_lm_loss_fwd
# =====================================================================================================================
LMF_PATTERNS = ("gauss", "sat", "equal", "asc", "desc", "outlier", "dup_trip", "dup_lane", "dup_wave", "max0", "maxlast", "neginf")
LMF_ENTRIES = (0, 1, 3, 300)
LMF_ROUTES = ("vec", "vec_pad8", "scalar:ld%4", "scalar:base")


def lmf_case(i):
    V = LM_V[i % 13]
    ls = LM_SMOOTH[(i // 13 + i) % 3] if V >= 3 else 0.0
    route = LMF_ROUTES[(i // 13) % 4]
    if V == WORKLOAD_V:
        route = ("vec", "scalar:base")[(i // 13) % 2]
    ld = {"vec": up(V, 4), "vec_pad8": up(V, 4) + 8, "scalar:ld%4": up(V, 4) + 1 + (i // 52) % 3, "scalar:base": up(V, 4)}[route]
    if V == WORKLOAD_V:
        ld = WORKLOAD_LD
    return dict(fam="lmf", seed=400 + i, V=V, ld=ld, off=1 if route == "scalar:base" else 0, ls=ls, hit=bool((i // 2) % 2 == 0), rot=i % 12,
                rows=WORKLOAD_ROWS if V == WORKLOAD_V else 12)


N_LMF = 78


def lmf_cases():
    return [lmf_case(i) for i in range(N_LMF)]


def lmf_vec(cfg):
    return cfg["ld"] % 4 == 0 and cfg["off"] % 4 == 0


def lmf_rows(cfg):
    """(wanted pattern, entries) of every row"""
    return [(LMF_PATTERNS[(cfg["rot"] + u) % 12], LMF_ENTRIES[(cfg["rot"] // 3 + u) % 4]) for u in range(cfg["rows"])]


def lmf_inputs(cfg):
    rs = np.random.RandomState(cfg["seed"])
    V, ld, ls = cfg["V"], cfg["ld"], cfg["ls"]
    vec = lmf_vec(cfg)
    logits = np.full((cfg["rows"], ld), 1e30, np.float32)
    pats, labels, ptr = [], [], [0]
    for u, (pat, ne) in enumerate(lmf_rows(cfg)):
        if pat == "neginf" and (ls > 0 or V < 4):
            pat = "gauss"
        z, pat = _lm_row(rs, V, pat, vec)
        avoid = ()
        if pat == "neginf":
            avoid = tuple(int(c) for c in rs.choice(np.arange(1, V), max(1, V // 5), replace=False))
            z[list(avoid)] = -np.inf
        logits[u, :V] = z
        pats.append(pat)
        labels.append(_lm_labels(rs, V, ne, avoid))
        ptr.append(ptr[-1] + ne)
    return dict(logits=logits, row_ptr=np.array(ptr, np.int32), labels=np.concatenate(labels).astype(np.int32), patterns=pats)


def lmf_branch(cfg):
    V, ls = cfg["V"], cfg["ls"]
    vec = lmf_vec(cfg)
    b = ["lmf_vec" if vec else ("lmf_scalar:ld%4" if cfg["ld"] % 4 else "lmf_scalar:base+1float")]
    span = VEC_STRIDE if vec else BLOCK
    b.append("lmf_one_trip" if V <= span else "lmf_trips>1")
    if vec:
        b.append("lmf_V%%4==%d" % (V % 4))
    b.append("lmf_pad_columns" if cfg["ld"] > V else "lmf_ld==V")
    b += ["lmf_ls=%g" % ls, "lmf_hit_given" if cfg["hit"] else "lmf_hit_null", "lmf_V<256" if V < BLOCK else "lmf_V>=256"]
    inp = lmf_inputs(cfg)
    for u, (_, ne) in enumerate(lmf_rows(cfg)):
        lab = inp["labels"][inp["row_ptr"][u]:inp["row_ptr"][u + 1]]
        b += ["lmf_row_" + inp["patterns"][u], "lmf_entries=%d" % ne]
        if 0 in lab:
            b.append("lmf_label0_ls=%g" % ls)
        if 1 in lab and V > 1:
            b.append("lmf_label_1")
        if V - 1 in lab and V > 2:
            b.append("lmf_label_V-1")
        if V % 4 and vec and np.any((lab >= 4 * (V // 4)) & (lab > 1)):
            b.append("lmf_label_in_last_partial_vector")
    return b


def lm_row_reference(z, lab, ls, vec):
    """one row of mv_lm_loss_fwd -> (loss, bound of the loss, M, S, relative bound of S) for the labels `lab`"""
    V = z.size
    smooth, conf, sval, _ = lm_const(ls, V)
    lab = np.asarray(lab, np.int64)
    loss, M, S, lse, logp = lm_row_loss(z, lab, ls)
    rel = lm_sum_relerr(z, vec)
    d_lse = (rel + ULP_LOG64 * 2 * U64 * abs(math.log(S)) + U64 * abs(lse)) * SLACK
    zt = z[lab].astype(np.float64)
    if smooth:
        # the closed form in double: its terms by their magnitudes, the lse error through c + (V - 2) s, one rounding to f32
        zs = np.abs(z[1:].astype(np.float64)).sum() if np.all(np.isfinite(z)) else 0.0
        mag = abs(conf) * (np.abs(zt) + abs(lse)) + sval * (zs + np.abs(zt) + (V - 2) * abs(lse)) + 20.0
        b = (conf + (V - 2) * sval) * d_lse + 8 * U64 * V * mag + U32 * np.abs(loss)
        b = np.where(lab == 0, 0.0, b)
    else:
        b = d_lse + U32 * np.abs(loss) + FLOOR
    return loss, b * SLACK, M, S, rel * SLACK


def lmf_reference(cfg, inp):
    V, ls = cfg["V"], cfg["ls"]
    vec = lmf_vec(cfg)
    n = int(inp["row_ptr"][-1])
    ref = dict(loss=np.zeros(n), loss_b=np.zeros(n), hit=np.zeros(n, np.int64), M=np.zeros(cfg["rows"], np.float32), S=np.zeros(cfg["rows"]),
               S_b=np.zeros(cfg["rows"]))
    for u in range(cfg["rows"]):
        z = inp["logits"][u, :V]
        e0, e1 = inp["row_ptr"][u], inp["row_ptr"][u + 1]
        lab = inp["labels"][e0:e1].astype(np.int64)
        ref["loss"][e0:e1], ref["loss_b"][e0:e1], ref["M"][u], ref["S"][u], rel = lm_row_reference(z, lab, ls, vec)
        ref["S_b"][u] = rel * ref["S"][u]
        ref["hit"][e0:e1] = lab == int(np.argmax(z))
    return ref


def lmf_restated(cfg, inp, defect=None):
    """the row in blocks of 128 columns, a block's sum first, then merged into the running (max, sum) -- another order than the kernel's"""
    V, ls, ld = cfg["V"], cfg["ls"], cfg["ld"]
    smooth, conf, sval, _ = lm_const(ls, V)
    n = int(inp["row_ptr"][-1])
    out = dict(loss=np.full(n, NAN, np.float32), hit=np.full(n, -7, np.int32) if cfg["hit"] else None, stat=np.zeros((cfg["rows"], 2), np.float32))
    Vr = min(up(V, 4), ld) if defect == "pad_unmasked" and lmf_vec(cfg) else V
    for u in range(cfg["rows"]):
        z = inp["logits"][u, :Vr]
        m, s = np.float32(-np.inf), 0.0
        for c0 in range(0, Vr, 128):
            blk = z[c0:c0 + 128]
            bm = blk.max()
            if not bm > -np.inf:
                continue
            bs = float(np.sum(np.exp(blk - bm).astype(np.float32).astype(np.float64)[::-1]))
            if bm > m:
                s = (s if defect == "no_rescale" else s * float(np.exp(np.float32(m - bm)))) + bs
                m = bm
            else:
                s += bs * float(np.exp(np.float32(bm - m)))
        sf = np.float32(s)
        out["stat"][u] = (m, sf)
        lse = float(m) + math.log(float(sf))
        zs = float(np.sum(z[(0 if defect == "zs_with_col0" else 1):].astype(np.float64)))
        am = int(np.argmax(z)) if defect != "tie_higher" else int(Vr - 1 - np.argmax(z[::-1]))
        e0, e1 = inp["row_ptr"][u], inp["row_ptr"][u + 1]
        for e in range(e0, min(e1, e0 + BLOCK) if defect == "entries_beyond_256_skipped" else e1):
            t = int(inp["labels"][e])
            zt = float(z[t])
            if not smooth:
                loss = lse - zt
            elif t == 0 and defect != "label0_counted":
                loss = 0.0
            else:
                nn = float(V - 2)
                loss = (conf * math.log(conf) if conf > 0 else 0.0) + nn * sval * math.log(sval) - conf * (zt - lse) - sval * ((zs - zt) - nn * lse)
            out["loss"][e] = loss
            if cfg["hit"]:
                out["hit"][e] = 1 if am == t else 0
    return out


def lmf_judge(cfg, inp, ref, out):
    v = Verdict()
    st = out["stat"].detach().cpu().numpy() if isinstance(out["stat"], torch.Tensor) else out["stat"]
    st = st.reshape(-1, 2)
    v.exact("row_stat[:, 0] bit-equal to the row maximum", np.array_equal(st[:, 0].astype(np.float32).view(np.int32), ref["M"].view(np.int32)))
    v.bounded("row_stat[:, 1]", st[:, 1], ref["S"], ref["S_b"])
    v.bounded("entry_loss", as64(out["loss"]), ref["loss"], ref["loss_b"])
    if cfg["hit"]:
        v.exact("entry_hit", np.array_equal(as64(out["hit"]), ref["hit"]))
    return v.result()


# =====================================================================================================================
# lms: mv_lm_loss_select
# =====================================================================================================================
LMS_B = (1, 2, 5, 255, 256, 257, 2048)
LMS_K = ("0", "1", "B-1", "B")
N_LMS = 56
LMS_GAP = 1e-9


def lms_case(i):
    B = LMS_B[i % 7]
    kk = LMS_K[(i // 7) % 4]
    return dict(fam="lms", seed=500 + i, B=B, k={"0": 0, "1": 1, "B-1": B - 1, "B": B}[kk], kname=kk, n0=(i % 11 == 3), hit=(i % 5 != 2),
                ties=(i % 3 != 1))


def lms_cases():
    return [lms_case(i) for i in range(N_LMS)]


def lms_inputs(cfg):
    rs = np.random.RandomState(cfg["seed"])
    B = cfg["B"]
    if cfg["n0"]:
        z = np.zeros(0, np.float32)
        return dict(loss=z, w=z.copy(), sample=np.zeros(0, np.int32), hits=np.zeros(0, np.int32) if cfg["hit"] else None, copies=[])
    per = [[] for _ in range(B)]                           # sample -> [(loss, weight, hit)]
    for b in range(B):
        if B > 2 and b % 7 == 3:
            continue                                       # a sample without entries
        for _ in range(rs.randint(1, 4)):
            per[b].append((np.float32(rs.uniform(0.05, 8.0)), np.float32(rs.choice([0.0, 0.25, 0.5, 0.75, 1.0, 1.0])), int(rs.rand() < 0.5)))
    copies = []
    if cfg["ties"] and B >= 5:
        for _ in range(max(1, B // 40)):                   # exact ties: a sample repeats another one's entries in their order
            a, b = sorted(rs.choice(B, 2, replace=False))
            if per[a]:
                per[b] = list(per[a])
                copies.append((int(a), int(b)))
    if B >= 2:
        per[B - 1] = [(np.float32(1.5), np.float32(0.0), 1), (np.float32(2.5), np.float32(0.0), 0)]          # zero weight, with and without a hit
    copies = [(a, b) for a, b in copies if per[a] and per[a] == per[b]]
    # entries interleaved: round j of every sample, samples in a drawn order -- a sample's own entries stay in their order
    order, ent = rs.permutation(B), []
    for j in range(3):
        ent += [(b,) + per[b][j] for b in order if len(per[b]) > j]
    return dict(loss=np.array([e[1] for e in ent], np.float32), w=np.array([e[2] for e in ent], np.float32),
                sample=np.array([e[0] for e in ent], np.int32), hits=np.array([e[3] for e in ent], np.int32) if cfg["hit"] else None, copies=copies)


def lms_branch(cfg):
    B = cfg["B"]
    inp = lms_inputs(cfg)
    b = ["lms_B<=256" if B <= BLOCK else "lms_sample_trips>1", "lms_k=" + cfg["kname"], "lms_hit_given" if cfg["hit"] else "lms_hit_null"]
    if B == SELECT_MAX_B:
        b.append("lms_B=cap")
    if inp["w"].size == 0:
        return b + ["lms_n=0"]
    if len(set(inp["sample"].tolist())) < B:
        b.append("lms_sample_without_entries")
    if inp["copies"]:
        b.append("lms_exact_ties")
    if inp["hits"] is not None and np.any((inp["w"] == 0) & (inp["hits"] == 1)):
        b.append("lms_zero_weight_with_hit")
    if np.any((inp["w"] == 0) & ((inp["hits"] == 0) if inp["hits"] is not None else True)):
        b.append("lms_zero_weight_without_hit")
    return b


def lms_sums(inp, B):
    """math.fsum per sample of the exact products w * loss -> (loss sums, weight sums, hits), python floats / ints"""
    prod, wts, hit = [[] for _ in range(B)], [[] for _ in range(B)], [0] * B
    for e in range(inp["w"].size):
        b = int(inp["sample"][e])
        prod[b].append(float(inp["w"][e]) * float(inp["loss"][e]))
        wts[b].append(float(inp["w"][e]))
        if inp["w"][e] > 0 and inp["hits"] is not None and inp["hits"][e]:
            hit[b] += 1
    return [math.fsum(p) for p in prod], [math.fsum(w) for w in wts], hit


def lms_reference(cfg, inp):
    B, k = cfg["B"], cfg["k"]
    L, W, H = lms_sums(inp, B)
    order = sorted(range(B), key=lambda b: (L[b], b))[:k]
    keep = np.zeros(B, np.int64)
    keep[order] = 1
    ls, ws = math.fsum(L[b] for b in order), math.fsum(W[b] for b in order)
    den = ws + 1e-5
    vals = np.array([ls / den, ws, 1.0 / den])
    # one rounding to f32 of a value formed in double from at most n + B double additions
    return dict(keep=keep, cnt=len(order), hits=sum(H[b] for b in order), vals=vals, vals_b=np.abs(vals) * (U32 + 4 * (inp["w"].size + B + 4) * U64) + FLOOR)


def lms_restated(cfg, inp, defect=None):
    B, k, n = cfg["B"], cfg["k"], inp["w"].size
    w, l, s = inp["w"].astype(np.float64), inp["loss"].astype(np.float64), inp["sample"]
    L = np.bincount(s, weights=w * l, minlength=B) if n else np.zeros(B)
    W = np.bincount(s, weights=w, minlength=B) if n else np.zeros(B)
    h = inp["hits"] if inp["hits"] is not None else np.zeros(n, np.int32)
    hm = (h != 0) if defect == "hits_zero_weight" else ((h != 0) & (w > 0))
    H = np.bincount(s, weights=hm.astype(np.float64), minlength=B) if n else np.zeros(B)
    idx = np.arange(B)
    order = np.lexsort((idx if defect != "tie_higher" else -idx, L if defect != "k_largest" else -L))[:k]
    keep = np.zeros(B, np.int32)
    keep[order] = 1
    den = W[order].sum() + (0.0 if defect == "no_1e-5" else 1e-5)
    with np.errstate(divide="ignore", invalid="ignore"):
        stats = np.array([L[order].sum() / den, W[order].sum(), len(order), H[order].sum()]).astype(np.float32)
        inv = np.array([1.0 / den]).astype(np.float32)
    return dict(keep=keep, stats=stats, inv=inv)


def lms_judge(cfg, inp, ref, out):
    v = Verdict()
    st = as64(out["stats"]).reshape(-1)
    v.exact("keep", np.array_equal(as64(out["keep"]).reshape(-1), ref["keep"]))
    v.exact("count", st[2] == ref["cnt"])
    v.exact("hits", st[3] == ref["hits"])
    v.bounded("stats[0], stats[1], inv_denom", [st[0], st[1], as64(out["inv"]).reshape(-1)[0]], ref["vals"], ref["vals_b"])
    return v.result()


# =====================================================================================================================
# lmb: mv_lm_loss_bwd (and lmchain: fwd -> select -> bwd)
# =====================================================================================================================
LMB_ROUTES = ("vec", "vec_ldd=ld+8", "scalar:ld%4", "scalar:ldd%4", "scalar:logits_base", "scalar:d_base", "vec:d_base+8B")
LMB_ROWS = ("noentry", "alldropped", "allzeroweight", "alllabel0", "mixed", "same3", "two_in_vec", "specials")
LMB_B = 6
LMB_KEEP = (1, 0, 1, 1, 0, 1)
N_LMB = 91


def lmb_case(i):
    V = LM_V[i % 13]
    route = LMB_ROUTES[(i // 13) % 7]
    ddt = (F32, BF16, F16)[(i // 13 + i) % 3]
    if route == "vec:d_base+8B":
        ddt = BF16 if i % 2 else F16
    ld = up(V, 4) + (1 if route == "scalar:ld%4" else 0) + (4 if (i // 5) % 2 else 0)
    if V == WORKLOAD_V:
        ld = WORKLOAD_LD + (1 if route == "scalar:ld%4" else 0)
    ldd = {"vec": (up(V, 4), ld)[i % 2], "vec_ldd=ld+8": ld + 8, "scalar:ld%4": up(V, 4), "scalar:ldd%4": V if V % 4 else V + 1, "scalar:logits_base": ld,
           "scalar:d_base": up(V, 4), "vec:d_base+8B": ld}[route]
    ls = LM_SMOOTH[(i // 13 + i // 39) % 3] if V >= 3 else 0.0
    return dict(fam="lmb", seed=600 + i, V=V, ld=ld, ldd=ldd, ddt=ddt, l_off=1 if route == "scalar:logits_base" else 0,
                d_off=1 if route == "scalar:d_base" else 4 if route == "vec:d_base+8B" else 0, ls=ls, lsdev=bool((i // 3) % 2))


def lmb_cases():
    return [lmb_case(i) for i in range(N_LMB)]


def lmb_vec(cfg):
    return cfg["ld"] % 4 == 0 and cfg["ldd"] % 4 == 0 and (cfg["l_off"] * 4) % 16 == 0 and (cfg["d_off"] * ESIZE[cfg["ddt"]]) % (4 * ESIZE[cfg["ddt"]]) == 0


def lmb_inputs(cfg, chain=False):
    rs = np.random.RandomState(cfg["seed"])
    V, ld, ls = cfg["V"], cfg["ld"], cfg["ls"]
    vec = lmb_vec(cfg)
    kept, dropped = [b for b in range(LMB_B) if LMB_KEEP[b]], [b for b in range(LMB_B) if not LMB_KEEP[b]]
    logits = np.full((len(LMB_ROWS), ld), 1e30, np.float32)
    lab, wt, smp, ptr, why = [], [], [], [0], []
    for u, kind in enumerate(LMB_ROWS):
        z, _ = _lm_row(rs, V, ("gauss", "sat", "outlier", "gauss")[(u + cfg["seed"]) % 4], vec)
        logits[u, :V] = z
        wgt = lambda: float(rs.choice([0.25, 0.5, 0.75, 1.0]))                                  # noqa: E731
        if kind == "noentry":
            ent = []
        elif kind == "alldropped":
            ent = [(int(c), wgt(), dropped[j % 2]) for j, c in enumerate(_lm_labels(rs, V, 3))]
        elif kind == "allzeroweight":
            ent = [(int(c), 0.0, kept[j % 4]) for j, c in enumerate(_lm_labels(rs, V, 2))]
        elif kind == "alllabel0":
            ent = [(0, wgt(), kept[0]), (0, wgt(), kept[1])]
        elif kind == "mixed":
            ent = [(int(c), wgt(), (kept + dropped)[j % 6]) for j, c in enumerate(_lm_labels(rs, V, 6))]
        elif kind == "same3":
            c = int(rs.randint(1, V)) if V > 1 else 0
            ent = [(c, wgt(), kept[0]), (c, wgt(), dropped[0]), (c, wgt(), kept[2]), (c, wgt(), kept[1])]
        elif kind == "two_in_vec":
            c = 4 * int(rs.randint(0, max(V // 4, 1)))
            ent = [(min(c + 1, V - 1), wgt(), kept[0]), (min(c + 3, V - 1), wgt(), kept[3]), (min(c + 1, V - 1), 0.0, kept[1])]
        else:
            ent = [(int(c), wgt(), kept[j % 4]) for j, c in enumerate(_lm_labels(rs, V, 8))]
        cf = [w if LMB_KEEP[s] else 0.0 for (_, w, s) in ent]
        dead = not any(c > 0 and not (ls > 0 and t == 0) for c, (t, _, _) in zip(cf, ent))
        why.append(kind if dead else None)
        if dead and not chain:
            logits[u, :] = NAN                             # "no logit is read"
        lab += [e[0] for e in ent]
        wt += [e[1] for e in ent]
        smp += [e[2] for e in ent]
        ptr.append(len(lab))
    inp = dict(logits=logits, row_ptr=np.array(ptr, np.int32), labels=np.array(lab, np.int32), w=np.array(wt, np.float32),
               sample=np.array(smp, np.int32), keep=np.array(LMB_KEEP, np.int32), g=f32r(0.5), lsv=256.0 if cfg["lsdev"] else None, dead=why)
    if not chain:
        wkept = math.fsum(float(w) for w, s in zip(wt, smp) if LMB_KEEP[s])
        inp["inv"] = np.array([1.0 / (wkept + 1e-5)], np.float32)
        stat = np.zeros((len(LMB_ROWS), 2), np.float32)
        for u in range(len(LMB_ROWS)):
            if why[u] is None:
                zz = logits[u, :V].astype(np.float64)
                stat[u] = (zz.max(), math.fsum(np.exp(zz - zz.max())))
            else:
                stat[u] = NAN
        inp["stat"] = stat
    return inp


def lmb_branch(cfg):
    V, ld, ldd = cfg["V"], cfg["ld"], cfg["ldd"]
    b = ["lmb_d_" + cfg["ddt"], "lmb_ls=%g" % cfg["ls"], "lmb_loss_scale_given" if cfg["lsdev"] else "lmb_loss_scale_null"]
    if lmb_vec(cfg):
        b.append("lmb_vec")
        if cfg["d_off"]:
            b.append("lmb_vec:d_base+8B")
    else:
        b += ["lmb_scalar:" + n for n, c in (("ld%4", ld % 4), ("ldd%4", ldd % 4), ("logits_base", cfg["l_off"]), ("d_base", cfg["d_off"] % 4)) if c]
        b.append("lmb_scalar")
    b.append("lmb_ldd==V" if ldd == V else "lmb_ldd==up(V,4)" if ldd == up(V, 4) else "lmb_ldd==ld" if ldd == ld else "lmb_ldd==ld+8" if ldd == ld + 8 else "lmb_ldd_other")
    if ldd != ld:
        b.append("lmb_ldd!=ld")
    b.append("lmb_one_trip" if ldd <= (VEC_STRIDE if lmb_vec(cfg) else BLOCK) else "lmb_trips>1")
    inp = lmb_inputs(cfg)
    b += ["lmb_!any:" + w for w in inp["dead"] if w]
    lab = inp["labels"]
    for name, c in (("0", 0), ("1", 1), ("V-1", V - 1), ("1023", 1023), ("1024", 1024)):
        if c in lab and c < V:
            b.append("lmb_label_" + name + ("_plain" if name == "0" and cfg["ls"] == 0 else ""))
    if np.any(lab > 1024):
        b.append("lmb_label>1024")
    return b + ["lmb_row_mixed", "lmb_row_same3", "lmb_row_two_in_vec"]


def lmb_reference(cfg, inp, chain=None):
    """fp64 gradient [U, V] and its bound.  chain: None, or dict(keep, inv, p_rel [U], g_rel) -- the values and extra relative errors of
    the quantities that mv_lm_loss_bwd takes from the forward and selection kernels instead of from this reference"""
    V, ls = cfg["V"], cfg["ls"]
    smooth, conf, sval, qsum = lm_const(ls, V)
    conf32 = f32r(conf)
    U = len(LMB_ROWS)
    keep = inp["keep"] if chain is None else chain["keep"]
    inv = float(inp["inv"][0]) if chain is None else chain["inv"]
    G = float(inp["g"]) * (inp["lsv"] or 1.0) * inv
    hot = (conf32 - sval) if smooth else 1.0
    grad, bound, dead = np.zeros((U, V)), np.zeros((U, V)), []
    for u in range(U):
        e0, e1 = inp["row_ptr"][u], inp["row_ptr"][u + 1]
        ent = [(int(inp["labels"][e]), float(inp["w"][e]) if keep[inp["sample"][e]] else 0.0) for e in range(e0, e1)]
        live = [(t, cf) for t, cf in ent if cf > 0 and not (smooth and t == 0)]
        dead.append(not live)
        if not live:
            continue
        ne = len(live)
        amass, wsm = sum(cf * qsum for _, cf in live), sum(cf for _, cf in live)
        z = inp["logits"][u, :V].astype(np.float64)
        if chain is None:
            M, S = float(inp["stat"][u, 0]), float(inp["stat"][u, 1])
        else:
            M = z.max()
            S = math.fsum(np.exp(z - M))
        d = np.where(np.isfinite(z), M - z, 0.0)
        p = np.where(np.isfinite(z), np.exp(-d), 0.0) / S
        T1 = amass * p
        base = np.full(V, sval * wsm if smooth else 0.0)
        base[0] = 0.0
        Hc, cnt = np.zeros(V), np.zeros(V)
        for t, cf in live:
            Hc[t] += cf * hot
            cnt[t] += 1
        r = T1 - base - Hc
        mags = np.abs(T1) + np.abs(base) + Hc
        p_rel = E_EXP + U32 * d + E_DIV + U32 + (chain["p_rel"][u] if chain else 0.0)
        b = T1 * (p_rel + (ne + 2) * U32) + base * (ne + 2) * U32 + Hc * 2 * U32 + (1 + cnt) * U32 * mags
        g_rel = 3 * U32 + (chain["g_rel"] if chain else 0.0)
        grad[u], bound[u] = r * G, abs(G) * (b + g_rel * mags)
    return dict(grad=grad, grad_b=store_bound(grad, bound, cfg["ddt"]), dead=dead)


def lmb_restated(cfg, inp, defect=None):
    V, ls, ldd = cfg["V"], cfg["ls"], cfg["ldd"]
    smooth, conf, sval, qsum = lm_const(ls, V)
    f = np.float32
    U = len(LMB_ROWS)
    out = np.full((U, ldd), NAN, np.float32)
    G = f(inp["g"]) * (f(inp["lsv"]) if inp["lsv"] is not None else f(1.0)) * inp["inv"][0]
    hot = f(f(conf) - f(sval)) if smooth else f(1.0)
    for u in range(U):
        e0, e1 = inp["row_ptr"][u], inp["row_ptr"][u + 1]
        ent = [(int(inp["labels"][e]), f(inp["w"][e]) if (inp["keep"][inp["sample"][e]] or defect == "dropped_contribute") else f(0.0))
               for e in range(e0, e1)]
        live = [(t, cf) for t, cf in ent if cf > 0 and not (smooth and t == 0)]
        if not live:
            out[u, :(V if defect == "any_pad_unwritten" else ldd)] = 0.0
            continue
        amass, wsm = f(0.0), f(0.0)
        for _, cf in reversed(live):
            amass, wsm = f(amass + cf * f(qsum)), f(wsm + cf)
        z = inp["logits"][u, :V]
        M, inv_s = inp["stat"][u, 0], f(1.0) / inp["stat"][u, 1]
        o = amass * (np.exp(z - M).astype(np.float32) * inv_s)
        base = np.full(V, f(sval) * wsm if smooth else f(0.0), np.float32)
        if defect != "sval_in_col0":
            base[0] = 0.0
        if defect == "no_smoothing_ge_1024":
            base[VEC_STRIDE:] = 0.0
        o = o - base
        seen = set()
        for t, cf in live:
            if defect == "repeat_counted_once" and t in seen:
                continue
            seen.add(t)
            o[t] = o[t] - cf * hot
        out[u, :V] = o * G
        out[u, V:] = 0.0
    return dict(dlogits=to_enc(out, cfg["ddt"]))


def lmb_judge(cfg, inp, ref, out):
    """out["dlogits"]: [U, ldd]; out["guards_ok"] (GPU runner only): the elements around the buffer kept their bits"""
    v, V = Verdict(), cfg["V"]
    g = as64(out["dlogits"]).reshape(len(LMB_ROWS), cfg["ldd"])
    dead = np.array(ref["dead"])
    v.exact("rows without a live entry: every one of the ldd columns exactly zero", np.all(g[dead] == 0.0))
    v.exact("pad columns V..ldd-1 exactly zero", np.all(g[:, V:] == 0.0))
    v.bounded("dlogits", g[~dead][:, :V], ref["grad"][~dead], ref["grad_b"][~dead])
    v.exact("guards", out.get("guards_ok", True))
    return v.result()


def old_scheme_passes(cfg, inp, ref, out):
    """the tolerance the hand-picked tests apply (tests/test_report_finetune_gpu.py: GTOL x total scale, largest absolute error)"""
    gtol = {F32: 1e-6, BF16: 2e-2, F16: 3e-3}[cfg["ddt"]]
    g = as64(out["dlogits"]).reshape(len(LMB_ROWS), cfg["ldd"])[:, :cfg["V"]]
    live = ~np.array(ref["dead"])
    err = float(np.max(np.abs(g[live] - ref["grad"][live])))
    return err < gtol * float(inp["g"]) * (inp["lsv"] or 1.0), err


# ---- lmchain ----------------------------------------------------------------------------------------------------------
LMCHAIN_K = 4
N_LMCHAIN = 12


def lmchain_cases():
    pick = [i for i in range(N_LMB) if lmb_case(i)["V"] >= 5][::6][:N_LMCHAIN]
    return [dict(lmb_case(i), fam="lmchain", seed=701 + i) for i in pick]


def lmchain_branch(cfg):
    return ["lmchain_" + ("vec" if lmb_vec(cfg) else "scalar"), "lmchain_d_" + cfg["ddt"], "lmchain_ls=%g" % cfg["ls"]]


def lmchain_inputs(cfg):
    return lmb_inputs(cfg, chain=True)


def lmchain_reference(cfg, inp):
    """fwd -> select -> bwd in fp64 from the logits alone; the backward's bound widened by what the forward's row sums and the
    selection's 1 / denominator carry"""
    V, ls = cfg["V"], cfg["ls"]
    vec_f = cfg["ld"] % 4 == 0 and cfg["l_off"] == 0
    n = inp["labels"].size
    loss, loss_b, p_rel = np.zeros(n), np.zeros(n), np.zeros(len(LMB_ROWS))
    for u in range(len(LMB_ROWS)):
        e0, e1 = inp["row_ptr"][u], inp["row_ptr"][u + 1]
        loss[e0:e1], loss_b[e0:e1], _, _, rel = lm_row_reference(inp["logits"][u, :V], inp["labels"][e0:e1], ls, vec_f)
        p_rel[u] = rel + E_DIV
    sel = dict(loss=loss.astype(np.float32), w=inp["w"], sample=inp["sample"], hits=None)
    L, W, _ = lms_sums(dict(sel, loss=loss), LMB_B)
    order = sorted(range(LMB_B), key=lambda b: (L[b], b))[:LMCHAIN_K]
    keep = np.zeros(LMB_B, np.int32)
    keep[order] = 1
    den = math.fsum(W[b] for b in order) + 1e-5
    ref = lmb_reference(cfg, inp, chain=dict(keep=keep, inv=1.0 / den, p_rel=p_rel, g_rel=2 * U32))
    # the scalar loss: every kept entry's loss within its bound, weighted; double sums; one rounding to f32
    w = inp["w"].astype(np.float64) * keep[inp["sample"]]
    val = math.fsum(L[b] for b in order) / den
    ref.update(keep=keep, sums=L, loss=val, loss_b=(float(np.sum(w * loss_b)) / den + (U32 + 4 * (n + LMB_B) * U64) * abs(val)) * SLACK + FLOOR)
    return ref


def lmchain_restated(cfg, inp, defect=None):
    fcfg = dict(cfg, rows=len(LMB_ROWS), hit=False)
    f = lmf_restated(fcfg, inp)
    s = lms_restated(dict(B=LMB_B, k=LMCHAIN_K), dict(loss=f["loss"], w=inp["w"], sample=inp["sample"], hits=None))
    out = lmb_restated(cfg, dict(inp, keep=s["keep"], inv=s["inv"], stat=f["stat"]), defect)
    return dict(out, keep=s["keep"], stats=s["stats"])


def lmchain_judge(cfg, inp, ref, out):
    v = Verdict()
    v.exact("keep", np.array_equal(as64(out["keep"]).reshape(-1), ref["keep"]))
    ok, worst, what = lmb_judge(cfg, inp, ref, out)
    v.ok, v.worst, v.what = v.ok and ok, worst, v.what + ([what] if what else [])
    v.bounded("loss", as64(out["stats"]).reshape(-1)[:1], [ref["loss"]], [ref["loss_b"]])
    return v.result()


# =====================================================================================================================
# optim: mv_tensor_sqnorms, then mv_bertadam_step, twice
# =====================================================================================================================
OPTIM_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8195)
OPTIM_INACTIVE = (None, "first", "middle", "last")
OPTIM_SHADOWS = ("none", "bf16", "f16", "both")
OPTIM_STEPS = ("below", "at", "above", "past")
OPTIM_SCALER = ("none", "skip", "drive")
N_OPTIM = 48
SENT = {"p": 7.25, "m": -3.5, "v": 11.0, "g": 1e3}
NORM_DEPTH = 40     # additions on the longest path of the norm's summation tree: 16 per thread, 6 shuffles, 3 waves, then <= 1 + 6


def optim_case(i):
    rs = np.random.RandomState(9000 + i)
    T = 1 + (5 * i) % 12
    counts = tuple(OPTIM_COUNTS[(7 * i + 4 * j + j * j) % 15] for j in range(T))
    inactive = OPTIM_INACTIVE[i % 4] if T >= 3 else None
    sched = SCHEDULES[(i // 2) % 3]
    return dict(fam="optim", seed=800 + i, counts=counts, decay=tuple(int(x) for x in rs.randint(0, 2, T)), inactive=inactive, gap2=bool((i // 3) % 2),
                tail=bool(i % 2), shadows=OPTIM_SHADOWS[(i // 4) % 4], mgn=(-1.0, 1.0)[(i // 2 + i) % 2], sched=sched,
                t_total=-1 if i % 8 == 5 else 10, where=OPTIM_STEPS[(i // 4 + i) % 4], scaler=OPTIM_SCALER[(i // 5) % 3])


def optim_cases():
    return [optim_case(i) for i in range(N_OPTIM)]


def optim_layout(cfg):
    """-> (entries [(offset, count, decay, active)], n)"""
    T = len(cfg["counts"])
    off, ent = 0, []
    ia = {None: -1, "first": 0, "middle": T // 2, "last": T - 1}[cfg["inactive"]]
    for t, c in enumerate(cfg["counts"]):
        ent.append((off, c, bool(cfg["decay"][t]), t != ia))
        off = up(off + c, 64) + (64 if cfg["gap2"] and t % 2 else 0)
    end = ent[-1][0] + ent[-1][1]
    return ent, up(end, 4) + (128 if cfg["tail"] else 0)


def optim_tables(entries, chunk=OPTIM_CHUNK):
    """the tables optim.build_tables makes (the GPU file asserts they are the same)"""
    rows, ids = [], []
    for t, (off, cnt, decay, active) in enumerate(entries):
        rows.append([off, cnt, len(ids), (1 if decay else 0) | (2 if active else 0)])
        ids += [t] * ((cnt + chunk - 1) // chunk)
    return np.array(rows, np.int64).reshape(-1, 4), np.array(ids, np.int32)


def optim_hyper(cfg):
    warm, first = {"below": (0.35, 1), "at": (0.1, 1), "above": (0.1, 5), "past": (0.1, 10)}[cfg["where"]]
    return dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, warmup=warm, first_step=first)


def optim_branch(cfg):
    ent, n = optim_layout(cfg)
    b = ["optim_T=%d" % len(ent)] if len(ent) in (1, 12) else []
    for off, c, decay, active in ent:
        b.append("optim_count=%d" % c)
        if active:
            b.append("optim_tail_%d" % (c % 4) if c % 4 else "optim_whole_vectors")
            b.append("optim_decay_on" if decay else "optim_decay_off")
            b.append("optim_chunks=%d" % ((c + OPTIM_CHUNK - 1) // OPTIM_CHUNK))
    b.append("optim_inactive_" + str(cfg["inactive"]).lower())
    b.append("optim_n_with_tail_gap" if cfg["tail"] else "optim_n_smallest")
    b += ["optim_shadows_" + cfg["shadows"], "optim_clip_on" if cfg["mgn"] > 0 else "optim_clip_off", "optim_" + cfg["sched"],
          "optim_t_total=-1" if cfg["t_total"] == -1 else "optim_step_" + cfg["where"], "optim_scaler_" + cfg["scaler"], "optim_two_steps"]
    if cfg["mgn"] > 0:
        inp = optim_inputs(cfg)
        sq = [float((inp["g"][o:o + c].astype(np.float64) ** 2).sum()) for o, c, _, a in ent if a]
        b += ["optim_some_tensor_clips"] * any(s > 1.0 for s in sq) + ["optim_some_tensor_does_not_clip"] * any(s < 1.0 for s in sq)
    return b


def optim_inputs(cfg):
    rs = np.random.RandomState(cfg["seed"])
    ent, n = optim_layout(cfg)
    st = {k: np.full(n, SENT[k], np.float32) for k in "pgmv"}
    for t, (off, c, _, _) in enumerate(ent):
        st["p"][off:off + c] = rs.randn(c)
        norm = (0.3, 3.0)[t % 2] if cfg["mgn"] > 0 else math.sqrt(c)       # with clipping: tensors on either side of max_grad_norm
        g = rs.randn(c)
        st["g"][off:off + c] = g * norm / max(np.linalg.norm(g), 1e-3)
        st["m"][off:off + c] = 0.0
        st["v"][off:off + c] = 0.0
    st["sh_bf16"] = to_enc(np.full(n, 9.0), BF16) if cfg["shadows"] in ("bf16", "both") else None
    st["sh_f16"] = to_enc(np.full(n, 9.0), F16) if cfg["shadows"] in ("f16", "both") else None
    return st


def optim_lr(cfg, step):
    """bertadam_lr(): python floats are doubles; one rounding to f32"""
    h = optim_hyper(cfg)
    if cfg["t_total"] == -1:
        return f32r(h["lr"])
    x = step / cfg["t_total"]
    if x < h["warmup"]:
        f = x / h["warmup"]
    elif cfg["sched"] == "warmup_constant":
        f = 1.0
    elif cfg["sched"] == "warmup_cosine":
        f = 0.5 * (1.0 + math.cos(math.pi * x))
    else:
        f = max((x - 1.0) / (h["warmup"] - 1.0), 0.0)
    return f32r(h["lr"] * f)


def optim_reference(cfg, st, k):
    """update k (0 / 1) in fp64 from the f32 state `st` (dict p, g, m, v) -> dict of p, m, v, sq with bounds and the mask of elements
    an update may touch"""
    h = optim_hyper(cfg)
    ent, n = optim_layout(cfg)
    b1, omb1, b2, omb2, eps, wd0 = f32r(h["b1"]), f32r(1.0 - h["b1"]), f32r(h["b2"]), f32r(1.0 - h["b2"]), f32r(h["eps"]), f32r(h["wd"])
    lr_t = optim_lr(cfg, h["first_step"] + k)
    ref = {x: st[x].astype(np.float64).copy() for x in "pmv"}
    bnd = {x: np.zeros(n) for x in "pmv"}
    live = np.zeros(n, bool)
    sq, sq_b = np.zeros(len(ent)), np.zeros(len(ent))
    for t, (off, c, decay, active) in enumerate(ent):
        if not active:
            continue
        sl = slice(off, off + c)
        p, g, m, v = (st[x][sl].astype(np.float64) for x in "pgmv")
        s = float((g * g).sum())
        sq[t], sq_b[t] = s, (U32 * s + min(c, NORM_DEPTH) * U32 * s) * SLACK + FLOOR
        clip, d_clip = 1.0, 0.0
        if cfg["mgn"] > 0:
            ratio = f32r(cfg["mgn"]) / (math.sqrt(s) + f32r(1e-6))
            clip = min(ratio, 1.0)
            d_clip = (0.5 * sq_b[t] / max(s, 1e-300) + E_SQRT + U32 + E_DIV) if ratio < 1.0 + 1e-3 else 0.0
        if cfg["scaler"] == "skip":
            continue
        live[sl] = True
        gc = g * clip
        d_gc = np.abs(gc) * (U32 + d_clip)
        m2 = b1 * m + omb1 * gc
        d_m = U32 * (np.abs(b1 * m) + np.abs(omb1 * gc) + np.abs(m2)) + omb1 * d_gc
        v2 = b2 * v + omb2 * gc * gc
        d_v = U32 * (np.abs(b2 * v) + np.abs(v2)) + omb2 * gc * gc * (2 * U32 + 2 * (U32 + d_clip))
        rt = np.sqrt(v2)
        d_rt = np.where(v2 > 0, 0.5 * d_v / np.maximum(rt, 1e-300), np.sqrt(d_v)) + E_SQRT * rt
        den = rt + eps
        d_den = d_rt + U32 * den
        u = m2 / den
        d_u = d_m / den + np.abs(u) * d_den / den + E_DIV * np.abs(u)
        wd = wd0 if decay else 0.0
        u2 = u + wd * p
        d_u2 = d_u + (U32 * (np.abs(wd * p) + np.abs(u2)) if wd > 0 else 0.0)
        p2 = p - lr_t * u2
        # (the device's cos in double may differ in its last place from math.cos: the one rounding of lr_t to f32 may then fall the
        # other way, 2 U32 relative)
        d_p = abs(lr_t) * d_u2 + 3 * U32 * np.abs(lr_t * u2) + U32 * np.abs(p2)
        for x, val, d in (("p", p2, d_p), ("m", m2, d_m), ("v", v2, d_v)):
            ref[x][sl], bnd[x][sl] = val, d * SLACK + FLOOR
    return dict(ref=ref, bound=bnd, live=live, sq=sq, sq_b=sq_b, lr_t=lr_t)


def optim_restated(cfg, st, k, defect=None):
    """one update in numpy f32, a tensor at a time -> dict p, g, m, v, sh_bf16, sh_f16, sq"""
    f = np.float32
    h = optim_hyper(cfg)
    ent, n = optim_layout(cfg)
    b1, omb1, b2, omb2, eps = f(h["b1"]), f(1.0 - h["b1"]), f(h["b2"]), f(1.0 - h["b2"]), f(h["eps"])
    lr_t = f(optim_lr(cfg, h["first_step"] + k + (1 if defect == "step_off_by_one" else 0)))
    out = {x: (st[x].clone() if isinstance(st[x], torch.Tensor) else None if st[x] is None else st[x].copy()) for x in st}
    sq = np.zeros(len(ent), np.float32)
    for t, (off, c, decay, active) in enumerate(ent):
        if not active and defect != "inactive_updated":
            continue
        g = st["g"][off:off + c]
        gn = st["g"][off:min(up(off + c, 4), n)] if defect == "gap_in_norm" else g
        sq[t] = np.sum((gn * gn).astype(np.float32), dtype=np.float32)
        if cfg["scaler"] == "skip":
            continue
        clip = f(1.0)
        if cfg["mgn"] > 0:
            nrm = sq[t] if defect == "clip_squared" else np.sqrt(sq[t])
            clip = min(f(cfg["mgn"]) / f(nrm + f(1e-6)), f(1.0))
        cc = c - c % 4 if defect == "tail_not_updated" else c
        sl = slice(off, off + cc)
        p, g, m, v = (st[x][sl] for x in "pgmv")
        gc = g * clip
        m2 = b1 * m + omb1 * gc
        v2 = b2 * v + omb2 * gc * gc
        u = m2 / (np.sqrt(v2) + eps)
        if decay or defect == "decay_unflagged":
            u = u + f(h["wd"]) * p
        out["p"][sl], out["m"][sl], out["v"][sl] = p - lr_t * u, m2, v2
        for name, enc in (("sh_bf16", BF16), ("sh_f16", F16)):
            if out[name] is not None:
                out[name][sl] = to_enc(out["p"][sl], enc)
    out["sq"] = sq
    return out


def optim_judge(cfg, st, ref, out):
    """st: the state before the update, out: after it (numpy f32 p, g, m, v; torch 16-bit shadows or None; sq f32 [T])"""
    v = Verdict()
    ent, n = optim_layout(cfg)
    live = ref["live"]
    act = np.array([a for _, _, _, a in ent])
    if cfg["mgn"] > 0:
        v.bounded("sqnorms", as64(out["sq"])[act], ref["sq"][act], ref["sq_b"][act])
    for x in "pmv":
        got = np.asarray(out[x], np.float32)
        v.bounded(x, got[live], ref["ref"][x][live], ref["bound"][x][live])
        v.exact(x + ": gaps, inactive tensors (and everything under the skip flag) bit-unchanged",
                np.array_equal(got[~live].view(np.int32), np.asarray(st[x], np.float32)[~live].view(np.int32)))
    v.exact("g unchanged", np.array_equal(np.asarray(out["g"], np.float32).view(np.int32), np.asarray(st["g"], np.float32).view(np.int32)))
    lv = torch.from_numpy(live)
    pout = torch.from_numpy(np.ascontiguousarray(np.asarray(out["p"], np.float32)))
    for name, enc in (("sh_bf16", BF16), ("sh_f16", F16)):
        if st[name] is not None:
            got, was = out[name].cpu(), st[name].cpu()
            v.exact(name + ": the exact cast of the updated p", torch.equal(bits(got[lv]), bits(pout.to(DT[enc])[lv])))
            v.exact(name + ": untouched outside the updated tensors", torch.equal(bits(got[~lv]), bits(was[~lv])))
    return v.result()


# =====================================================================================================================
FAMILIES = {
    "rmul": (rmul_cases, rmul_branch), "bceml": (bceml_cases, bceml_branch), "bce": (bce_cases, bce_branch), "lmf": (lmf_cases, lmf_branch),
    "lms": (lms_cases, lms_branch), "lmb": (lmb_cases, lmb_branch), "lmchain": (lmchain_cases, lmchain_branch), "optim": (optim_cases, optim_branch),
}


def census(fam):
    """branch name -> number of cases of the family that reach it"""
    cases, branch = FAMILIES[fam]
    count = {}
    for c in cases():
        for b in set(branch(c)):
            count[b] = count.get(b, 0) + 1
    return count


def run_restated(cfg, defect=None):
    """a case through its restatement and judgement, as the GPU file runs it through the kernel -> (ok, worst error / bound, what)"""
    fam = cfg["fam"]
    if fam == "optim":
        st = optim_inputs(cfg)
        oks, worst, what = True, 0.0, []
        for k in range(2):
            ref = optim_reference(cfg, st, k)
            out = optim_restated(cfg, st, k, defect)
            ok, r, w = optim_judge(cfg, st, ref, out)
            oks, worst, what = oks and ok, max(worst, r), what + [w] * bool(w)
            st = {x: out[x] for x in st}
        return oks, worst, "; ".join(what)
    g = globals()
    inp = g[fam + "_inputs"](cfg)
    ref = g[fam + "_reference"](cfg, inp)
    return g[fam + "_judge"](cfg, inp, ref, g[fam + "_restated"](cfg, inp, defect))
