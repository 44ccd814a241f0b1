"""Case generators, dispatch predicates, fp64 references and error bounds of the sweep of the region encoder's support kernels
(csrc/mv_conv.hip: mv_nchw_to_nhwc, mv_im2col, mv_col_stats, mv_bn_finalize, mv_bn_act, mv_maxpool3x3s2).

Plain module: nothing here touches the GPU or the HIP library.  tests/test_convops_sweep_gpu.py runs the cases, and
tests/test_convops_cases_cpu.py counts which launcher branch every case takes, reads the caps below out of the .hip source, and shows
that the bounds let an honest f32 restatement through and catch each planted defect.

* every generator draws from np.random.RandomState(fixed + seed) and returns a dict; the tensors of a case are then made from
  cfg["seed"] alone (torch.Generator().manual_seed), so a cfg printed by a failing assertion reproduces the case;
* next to every generator stands a restatement of the launcher's dispatch, which names the branch(es) a case takes;
* the references are plain torch in float64 (float32 where the operation only moves data), on whatever device their inputs live;
  none of them calls a kernel of this project;
* the `*_restated` functions are the kernels written again in f32 (numpy / torch on the CPU, another summation order), with
  switches that plant one defect each: the CPU test runs them against the references under the bounds.

Alignment.  include/medvill.h states it: x / y / residual of mv_col_stats, mv_bn_act and mv_maxpool3x3s2 are aligned to four of their
elements, the f32 vectors of mv_bn_act to 16 bytes (the launchers refuse anything else).  Every base here is therefore offset by
whole vectors only: GUARD elements in front of an output.  mv_im2col looks at its bases itself and takes the scalar gather when they
are not 16-byte aligned, so one case moves its destination by 4 elements.
"""
import numpy as np
import torch
import torch.nn.functional as F

F32, BF16 = "f32", "bf16"
DT = {F32: torch.float32, BF16: torch.bfloat16}
ESIZE = {F32: 4, BF16: 2}
U32 = 2.0 ** -24                 # unit roundoff of f32
SLACK = 1.0 + 2.0 ** -10         # the first-order bounds below times this: second-order terms of a handful of roundings
NAN = float("nan")
GUARD = 16                       # elements in front of every output: a whole number of 16-byte vectors in both encodings
GUARD_ROWS = 2                   # rows behind every output

# ---- caps of the launchers (tests/test_convops_cases_cpu.py reads the same numbers out of csrc/mv_conv.hip) -------------------
GRID_CAP = 16384                 # grid_for(): blocks of the grid-stride kernels
THREADS = 256                    # threads per block, everywhere
SLAB_ROWS = 512                  # mv_col_stats: rows per slab until the cap binds
SLAB_CAP = 2048                  # mv_col_stats: at most this many slabs
COLS_PER_BLOCK = 64              # mv_col_stats: columns per block
ONE_TRIP = GRID_CAP * THREADS    # work items the grid covers in its first trip


def up(n, k):
    return (n + k - 1) // k * k


def cdiv(a, b):
    return (a + b - 1) // b


def f32r(x):
    """the value a C float argument holds"""
    return float(np.float32(x))


def within(got, ref, bound):
    """-> (ok, worst error / bound); a non-finite difference is never ok"""
    err = (got.double() - ref).abs()
    r = (err / (bound + 1e-300)).max()
    return bool(torch.isfinite(err).all()) and bool(r <= 1.0), float(r)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def half_ulp_bf16(a):
    """half a bf16 ulp at magnitude a (fp64 tensor): 2^(floor(log2 a) - 8); bf16 carries 8 significant bits"""
    return torch.exp2(torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126))) - 8.0)


# bf16 rounding (nearest even) of f32: ties in both directions and values just off a tie
T8 = 2.0 ** -8
BF16_SPECIALS = (1 + T8, 1 + 3 * T8, -(1 + T8), -(1 + 3 * T8), 1 + T8 + 2.0 ** -20, 1 + T8 - 2.0 ** -20, 1 + 3 * T8 - 2.0 ** -20,
                 255.5, 0.333, -2.5, 3.3895313892515355e38)


# =====================================================================================================================
# mv_nchw_to_nhwc
# =====================================================================================================================
NHWC_CHANNELS = ((3, 8), (5, 5))
NHWC_IMAGES = ((1, 1), (3, 5), (2, 7))
N_NHWC = 12


def nhwc_branches(cfg):
    """one kernel per output dtype; i < n grid-stride loop over B*H*W*Cp output elements"""
    b = ["nhwc_" + cfg["dt"], "nhwc_pad_channels" if cfg["Cp"] > cfg["C"] else "nhwc_Cp==C"]
    n = cfg["B"] * cfg["H"] * cfg["W"] * cfg["Cp"]
    b.append("nhwc_second_trip" if n > ONE_TRIP else "nhwc_one_trip")
    return b


def nhwc_case(seed):
    rs = np.random.RandomState(8000 + seed)
    C, Cp = NHWC_CHANNELS[seed % 2]
    H, W = NHWC_IMAGES[(seed // 4) % 3]
    return dict(fam="nhwc", seed=seed, dt=(BF16, F32)[(seed // 2) % 2], B=int(rs.randint(1, 4)), C=C, Cp=Cp, H=H, W=W)


NHWC_FIXED = [
    # just past 16384 * 256 output elements: 2 * 512 * 520 * 8 = 4,259,840
    dict(fam="nhwc", seed=8901, dt=BF16, B=2, C=3, Cp=8, H=512, W=520),
    dict(fam="nhwc", seed=8902, dt=F32, B=2, C=3, Cp=8, H=512, W=520),
]


def nhwc_cases():
    return [nhwc_case(s) for s in range(N_NHWC)] + NHWC_FIXED


def _plant_specials(flat, seed):
    sp = torch.tensor(BF16_SPECIALS, dtype=torch.float32).roll(seed % len(BF16_SPECIALS))
    k = min(flat.numel(), sp.numel())
    flat[:k] = sp[:k]
    if flat.numel() > 2 * sp.numel():
        flat[flat.numel() - sp.numel():] = sp.roll(3)


def nhwc_inputs(cfg):
    """f32 pixels [B, C, H, W] carrying the bf16 rounding specials at both ends"""
    g = torch.Generator().manual_seed(cfg["seed"])
    x = torch.randn((cfg["B"], cfg["C"], cfg["H"], cfg["W"]), generator=g) * 2.0
    _plant_specials(x.view(-1), cfg["seed"])
    return x


def nhwc_reference(x, cfg):
    """[B*H*W, Cp] in the output encoding: the permutation, zero pad channels, one rounding"""
    B, C, H, W = x.shape
    out = torch.zeros((B, H, W, cfg["Cp"]), dtype=torch.float32, device=x.device)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out.to(DT[cfg["dt"]]).view(B * H * W, cfg["Cp"])


def nhwc_restated(x, cfg):
    """the kernel's index arithmetic: output element i -> (pixel, channel) -> source offset"""
    B, C, H, W = x.shape
    Cp, hw = cfg["Cp"], H * W
    i = torch.arange(B * hw * Cp)
    c, p = i % Cp, i // Cp
    b, yx = p // hw, p % hw
    src = x.reshape(-1)[torch.where(c < C, (b * C + c) * hw + yx, torch.zeros_like(i))]
    return torch.where(c < C, src, torch.zeros_like(src)).to(DT[cfg["dt"]]).view(B * hw, Cp)


# =====================================================================================================================
# mv_im2col
# =====================================================================================================================
# (kh, kw, stride, pad, H, W): the four convolution geometries of the trunk, the stem's on an image lower than its kernel, and one
# kernel that is not square (a tap index split by the wrong extent shows there)
IM2COL_GEOMS = ((7, 7, 2, 3, 9, 7), (3, 3, 1, 1, 9, 7), (3, 3, 2, 1, 9, 7), (1, 1, 2, 0, 9, 7), (7, 7, 2, 3, 5, 11), (1, 3, 1, 1, 4, 6))
TRUNK_KSP = ((7, 2, 3), (3, 1, 1), (3, 2, 1), (1, 2, 0))
# (dtype, C, ldk as a function of kc = kh*kw*C, elements the destination base is moved by)
IM2COL_VARIANTS = (
    (BF16, 8, lambda kc: kc, 0),                   # VEC8, no tail
    (BF16, 16, lambda kc: kc + 8, 0),              # VEC8, one whole group of tail
    (BF16, 3, lambda kc: kc, 0),                   # VEC4: C % 8
    (BF16, 12, lambda kc: up(kc, 8) + 8, 0),       # VEC4: C % 8, with a tail
    (BF16, 8, lambda kc: kc + 4, 0),               # VEC4: ldk % 8 == 4
    (F32, 4, lambda kc: kc, 0),                    # ldk % 4 == 0
    (F32, 3, lambda kc: up(kc, 4) + 1, 0),         # ldk % 4 == 1
    (F32, 5, lambda kc: up(kc, 4) + 3, 0),         # ldk % 4 == 3
    (BF16, 8, lambda kc: kc, 4),                   # VEC4: destination 8 bytes off 16-byte alignment
)


def im2col_shape(cfg):
    """-> (Ho, Wo, rows, kc)"""
    Ho = (cfg["H"] + 2 * cfg["pad"] - cfg["kh"]) // cfg["stride"] + 1
    Wo = (cfg["W"] + 2 * cfg["pad"] - cfg["kw"]) // cfg["stride"] + 1
    return Ho, Wo, cfg["B"] * Ho * Wo, cfg["kh"] * cfg["kw"] * cfg["C"]


def im2col_plan(cfg):
    """mv_im2col: (kernel, reasons the 8-wide gather was refused, column groups per row, work items)"""
    _, _, rows, _ = im2col_shape(cfg)
    C, ldk = cfg["C"], cfg["ldk"]
    if cfg["dt"] == F32:
        return "f32/VEC4", [], cdiv(ldk, 4), rows * cdiv(ldk, 4)
    why = []
    if C % 8:
        why.append("C%8")
    if ldk % 8:
        why.append("ldk%8")
    if ((GUARD + cfg["dst_off"]) * ESIZE[BF16]) % 16:
        why.append("misaligned")
    if why:
        return "bf16/VEC4", why, cdiv(ldk, 4), rows * cdiv(ldk, 4)
    return "bf16/VEC8", [], ldk // 8, rows * (ldk // 8)


def im2col_branches(cfg):
    kern, why, groups, items = im2col_plan(cfg)
    _, _, _, kc = im2col_shape(cfg)
    b = [kern] + ["VEC4:" + w for w in why]
    if kern != "bf16/VEC8":
        b.append("ldk_partial_last_group" if cfg["ldk"] % 4 else "ldk_whole_groups")
    b.append("ldk_pad_tail" if cfg["ldk"] > kc else "ldk==kc")
    b.append("im2col_second_trip" if items > ONE_TRIP else "im2col_one_trip")
    if cfg["kh"] == cfg["kw"] and (cfg["kh"], cfg["stride"], cfg["pad"]) in TRUNK_KSP:
        b.append("ksp=%d/%d/%d" % (cfg["kh"], cfg["stride"], cfg["pad"]))
    if cfg["H"] < cfg["kh"] or cfg["W"] < cfg["kw"]:
        b.append("image_smaller_than_kernel")
    if cfg["kh"] != cfg["kw"]:
        b.append("kh!=kw")
    return b


def im2col_case(seed):
    rs = np.random.RandomState(8100 + seed)
    kh, kw, s, p, H, W = IM2COL_GEOMS[seed % len(IM2COL_GEOMS)]
    dt, C, ldk_of, dst_off = IM2COL_VARIANTS[(seed // len(IM2COL_GEOMS)) % len(IM2COL_VARIANTS)]
    return dict(fam="im2col", seed=seed, dt=dt, B=int(rs.randint(1, 4)), H=H, W=W, C=C, kh=kh, kw=kw, stride=s, pad=p, ldk=ldk_of(kh * kw * C),
                dst_off=dst_off)


N_IM2COL = len(IM2COL_GEOMS) * len(IM2COL_VARIANTS)
IM2COL_FIXED = [
    # the 8-wide gather just past the grid cap: rows = 2 * 458 * 458 = 419,528, ten groups per row -> 4,195,280 > 16384 * 256
    dict(fam="im2col", seed=8911, dt=BF16, B=2, H=916, W=916, C=8, kh=3, kw=3, stride=2, pad=1, ldk=80, dst_off=0),
]


def im2col_cases():
    return [im2col_case(s) for s in range(N_IM2COL)] + IM2COL_FIXED


def im2col_inputs(cfg):
    """NHWC activation [B, H, W, C] in its encoding; no zeros, so that a pad column read from the image cannot pass for one"""
    g = torch.Generator().manual_seed(cfg["seed"])
    x = torch.randn((cfg["B"], cfg["H"], cfg["W"], cfg["C"]), generator=g)
    x = torch.where(x.abs() < 0.01, torch.full_like(x, 0.5), x)
    return x.to(DT[cfg["dt"]])


def im2col_reference(x, cfg):
    """F.unfold, re-ordered from (c, ky, kx) to (ky, kx, c), zero tail up to ldk.  -> [rows, ldk] in x's encoding"""
    B, H, W, C = x.shape
    Ho, Wo, rows, kc = im2col_shape(cfg)
    kk = cfg["kh"] * cfg["kw"]
    u = F.unfold(x.float().permute(0, 3, 1, 2), (cfg["kh"], cfg["kw"]), padding=cfg["pad"], stride=cfg["stride"])      # [B, C*kk, Ho*Wo]
    u = u.view(B, C, kk, Ho * Wo).permute(0, 3, 2, 1).reshape(rows, kc)
    out = torch.zeros((rows, cfg["ldk"]), dtype=torch.float32, device=x.device)
    out[:, :kc] = u
    return out.to(x.dtype)


def _tap_rows(n_out, n_in, k, stride, pad, defect):
    """source index of output position o under tap k: (clamped index, inside the image)"""
    o = torch.arange(n_out)
    i = (o - pad) * stride + k if defect == "stride_after_pad" else o * stride - pad + k
    return i.clamp(0, n_in - 1), (i >= 0) & (i < n_in)


def im2col_restated(x, cfg, defect=None):
    """The gather tap by tap, into a NaN-filled destination like the GPU test's.  defect: None, "taps_transposed", "edge_padding",
    "tail_unwritten", "stride_after_pad"."""
    B, H, W, C = x.shape
    Ho, Wo, rows, kc = im2col_shape(cfg)
    kh, kw = cfg["kh"], cfg["kw"]
    out = torch.full((B, Ho, Wo, cfg["ldk"]), NAN, dtype=x.dtype)
    if defect != "tail_unwritten":
        out[..., kc:] = 0.0
    for ky in range(kh):
        iy, vy = _tap_rows(Ho, H, ky, cfg["stride"], cfg["pad"], defect)
        for kx in range(kw):
            ix, vx = _tap_rows(Wo, W, kx, cfg["stride"], cfg["pad"], defect)
            v = x[:, iy][:, :, ix]                                    # [B, Ho, Wo, C]
            if defect != "edge_padding":
                v = torch.where((vy[:, None] & vx[None, :])[None, :, :, None], v, torch.zeros_like(v))
            tap = kx * kh + ky if defect == "taps_transposed" else ky * kw + kx
            out[..., tap * C:(tap + 1) * C] = v
    return out.view(rows, cfg["ldk"])


# =====================================================================================================================
# mv_maxpool3x3s2
# =====================================================================================================================
POOL_IMAGES = ((1, 1), (1, 7), (2, 2), (7, 1), (9, 7), (8, 6), (5, 8))
POOL_C = (4, 64)
N_POOL = len(POOL_IMAGES) * len(POOL_C) * 2


def pool_shape(cfg):
    Ho, Wo = (cfg["H"] - 1) // 2 + 1, (cfg["W"] - 1) // 2 + 1
    return Ho, Wo, cfg["B"] * Ho * Wo


def pool_branches(cfg):
    """one kernel per dtype, four channels per thread, grid-stride over B*Ho*Wo*(C/4)"""
    Ho, Wo, rows = pool_shape(cfg)
    b = ["pool_" + cfg["dt"], "pool_second_trip" if rows * (cfg["C"] // 4) > ONE_TRIP else "pool_one_trip"]
    b.append("pool_H_" + ("odd" if cfg["H"] % 2 else "even"))
    b.append("pool_W_" + ("odd" if cfg["W"] % 2 else "even"))
    if cfg["H"] == 1 or cfg["W"] == 1:
        b.append("pool_one_pixel_wide")
    return b


def pool_case(seed):
    rs = np.random.RandomState(8200 + seed)
    H, W = POOL_IMAGES[seed % len(POOL_IMAGES)]
    return dict(fam="pool", seed=seed, dt=(BF16, F32)[(seed // len(POOL_IMAGES)) % 2], B=int(rs.randint(1, 4)), H=H, W=W,
                C=POOL_C[(seed // (2 * len(POOL_IMAGES))) % len(POOL_C)])


POOL_FIXED = [
    # just past the grid cap: 2 * 1449 * 1449 = 4,199,202 output pixels of one channel group each
    dict(fam="pool", seed=8921, dt=BF16, B=2, H=2897, W=2897, C=4),
]


def pool_cases():
    return [pool_case(s) for s in range(N_POOL)] + POOL_FIXED


def pool_inputs(cfg):
    """NHWC [B, H, W, C], every value negative (never zero, never NaN), a fifth of the pixels -inf in some channel and the first
    image's top-left 3 x 3 corner -inf in every channel, so that whole windows hold nothing else."""
    g = torch.Generator().manual_seed(cfg["seed"])
    shape = (cfg["B"], cfg["H"], cfg["W"], cfg["C"])
    x = -(torch.randn(shape, generator=g).abs() * 3.0 + 0.25)
    x[torch.rand(shape, generator=g) < 0.2] = float("-inf")
    x[0, :3, :3, :] = float("-inf")
    return x.to(DT[cfg["dt"]])


def pool_reference(x, cfg):
    """max_pool2d(3, 2, 1) -> [B*Ho*Wo, C] in x's encoding (a maximum rounds nothing)"""
    y = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1)
    return y.permute(0, 2, 3, 1).reshape(-1, cfg["C"]).to(x.dtype)


def pool_restated(x, cfg, defect=None):
    """running maximum over the nine taps.  defect: None, "start_at_zero", "anchor_2oy"."""
    B, H, W, C = x.shape
    Ho, Wo, rows = pool_shape(cfg)
    xf = x.float()
    m = torch.full((B, Ho, Wo, C), 0.0 if defect == "start_at_zero" else float("-inf"))
    lead = 0 if defect == "anchor_2oy" else 1
    for ky in range(3):
        iy, vy = _tap_rows(Ho, H, ky, 2, lead, None)
        for kx in range(3):
            ix, vx = _tap_rows(Wo, W, kx, 2, lead, None)
            v = xf[:, iy][:, :, ix]
            v = torch.where((vy[:, None] & vx[None, :])[None, :, :, None], v, torch.full_like(v, float("-inf")))
            m = torch.maximum(m, v)
    return m.view(rows, C).to(x.dtype)


# =====================================================================================================================
# mv_col_stats
# =====================================================================================================================
STATS_ROWS = (1, 15, 16, 17, 31, 33, 511, 512, 513, 1000)
STATS_C = (4, 60, 64, 68, 256)
STATS_KINDS = ("int", "gauss", "gauss_offset")
STATS_INT_MAX_ROWS = 262144      # integers in [-8, 8]: 64 * rows <= 2^24, every partial sum exact in any order
N_STATS = 2 * len(STATS_ROWS) * len(STATS_C)


def stats_plan(rows):
    """mv_col_stats: (slabs the launcher wants, whether the cap binds, rows per block, blocks along the rows)"""
    want = cdiv(rows, SLAB_ROWS)
    slabs = min(want, SLAB_CAP)
    rpb = cdiv(rows, slabs)
    return slabs, want > SLAB_CAP, rpb, cdiv(rows, rpb)


def stats_walk_ends(rows):
    """How the 16 row lanes of a block end their walk (rows ry, ry + 16, ...: two per trip, then at most one): the set over all
    blocks of "pair", "single", "idle"."""
    _, _, rpb, gy = stats_plan(rows)
    ends = set()
    for length in {rpb if gy > 1 else rows, rows - (gy - 1) * rpb}:
        for ry in range(16):
            n = max(0, cdiv(length - ry, 16))
            ends.add("idle" if n == 0 else ("single" if n % 2 else "pair"))
    return ends


def stats_branches(cfg):
    rows, C = cfg["rows"], cfg["C"]
    slabs, capped, rpb, gy = stats_plan(rows)
    b = ["stats_" + cfg["dt"], "stats_" + cfg["kind"]]
    b.append("slab_cap_binds" if capped else ("slabs>1" if gy > 1 else "one_slab"))
    b.append("rpb<512" if rpb < SLAB_ROWS else ("rpb=512" if rpb == SLAB_ROWS else "rpb>512"))
    b += ["walk_ends_" + e for e in sorted(stats_walk_ends(rows))]
    if gy > 1 and rows % rpb:
        b.append("short_last_slab")
    b.append("last_column_block_partial" if C % COLS_PER_BLOCK else "column_blocks_whole")
    if C > COLS_PER_BLOCK:
        b.append("column_blocks>1")
    b.append("ldx>C" if cfg["ldx"] > C else "ldx==C")
    return b


def stats_case(seed):
    """two cases per (rows, C): the exactly summable one and a Gaussian one, dtype and row pitch alternating against each other"""
    rs = np.random.RandomState(8300 + seed)
    pair, second = seed // 2, seed % 2
    rows, C = STATS_ROWS[pair % len(STATS_ROWS)], STATS_C[(pair // len(STATS_ROWS)) % len(STATS_C)]
    flip = (pair + pair // len(STATS_ROWS)) % 2
    return dict(fam="stats", seed=seed, dt=(BF16, F32)[(flip + second) % 2], rows=rows, C=C, ldx=C + 4 * ((flip + second + int(rs.randint(2))) % 2),
                kind="int" if not second else STATS_KINDS[1 + pair % 2])


STATS_FIXED = [
    # past the slab cap (rows > 2048 * 512): 2048 slabs of 513 rows, the last one short
    dict(fam="stats", seed=8931, dt=BF16, rows=1050000, C=4, ldx=4, kind="int"),
    dict(fam="stats", seed=8932, dt=F32, rows=1050000, C=4, ldx=8, kind="int"),
    dict(fam="stats", seed=8933, dt=F32, rows=1048577, C=4, ldx=4, kind="gauss_offset"),
    # every lane ends on a pair in every slab, and a slab count that does not divide the rows
    dict(fam="stats", seed=8934, dt=F32, rows=1024, C=68, ldx=72, kind="int"),
    dict(fam="stats", seed=8935, dt=BF16, rows=12544, C=64, ldx=64, kind="gauss"),
]


def stats_cases():
    return [stats_case(s) for s in range(N_STATS)] + STATS_FIXED


def stats_int_range(rows):
    return 8 if rows <= STATS_INT_MAX_ROWS else 2


def stats_inputs(cfg):
    """x [rows, ldx] in its encoding, the pad columns NaN."""
    rows, C = cfg["rows"], cfg["C"]
    g = torch.Generator().manual_seed(cfg["seed"])
    if cfg["kind"] == "int":
        r = stats_int_range(rows)
        v = torch.randint(-r, r + 1, (rows, C), generator=g).float()
    else:
        v = torch.randn((rows, C), generator=g)
        if cfg["kind"] == "gauss_offset":
            v = v + torch.tensor([0.0, 1.0, -10.0, 100.0])[torch.arange(C) % 4]
    x = torch.full((rows, cfg["ldx"]), NAN)
    x[:, :C] = v
    return x.to(DT[cfg["dt"]])


def stats_reference(x, cfg):
    """-> (stats fp64 [2, C], bound fp64 [2, C]).  The bound is zero for the exactly summable inputs and the summation bound
    2 n 2^-24 sum|terms| otherwise (the square of a term is one of the n + 1 roundings the factor 2 n covers)."""
    v = x[:, :cfg["C"]].double()
    ref = torch.stack([v.sum(0), (v * v).sum(0)])
    if cfg["kind"] == "int":
        return ref, torch.zeros_like(ref)
    return ref, 2.0 * cfg["rows"] * U32 * torch.stack([v.abs().sum(0), (v * v).sum(0)])


def stats_restated(x, cfg, defect=None):
    """f32 sums row after row (the kernel adds lanes, slabs and atomics in another order).  defect: None, "row_dropped",
    "row_doubled", "last_column_block_skipped"."""
    C = cfg["C"]
    _, _, rpb, _ = stats_plan(cfg["rows"])
    v = x[:, :C].float().numpy()
    last = min(rpb, cfg["rows"]) - 1                       # the last row of the first slab
    if defect == "row_dropped":
        v = np.delete(v, last, axis=0)
    elif defect == "row_doubled":
        v = np.concatenate([v, v[last:last + 1]], axis=0)
    out = np.stack([v.sum(0, dtype=np.float32), (v * v).sum(0, dtype=np.float32)]) if v.shape[0] else np.zeros((2, C), np.float32)
    if defect == "last_column_block_skipped" and C % COLS_PER_BLOCK:
        out[:, C // COLS_PER_BLOCK * COLS_PER_BLOCK:] = 0.0
    return torch.from_numpy(out)


# =====================================================================================================================
# mv_bn_finalize
# =====================================================================================================================
FIN_C = (1, 255, 256, 257)
FIN_ROWS = (1, 2, 12544)
FIN_MOMENTUM = (0.1, 1.0)
FIN_EPS = (1e-5, 1e-3)
N_FIN = 2 * len(FIN_C) * len(FIN_ROWS)
FIN_CONST_VALUE = 3.0            # the constant column: mean 3, E[x^2] 9, variance 0, all exact in f32


def fin_branches(cfg):
    b = ["fin_rows=%d" % cfg["rows"], "fin_eps=%g" % cfg["eps"]]
    b += ["fin_running", "fin_running_momentum=%g" % cfg["momentum"]] if cfg["running"] else ["fin_no_running"]
    b.append("fin_blocks>1" if cfg["C"] > THREADS else "fin_one_block")
    if cfg["C"] % THREADS:
        b.append("fin_partial_last_block")
    b.append("fin_variance_0_column")                       # column 0 of every case (every column when rows == 1)
    return b


def fin_case(seed):
    rs = np.random.RandomState(8400 + seed)
    pair = seed // 2
    return dict(fam="fin", seed=seed, C=FIN_C[pair % len(FIN_C)], rows=FIN_ROWS[(pair // len(FIN_C)) % len(FIN_ROWS)], running=bool(seed % 2 == 0),
                momentum=FIN_MOMENTUM[(pair + int(rs.randint(2))) % 2], eps=FIN_EPS[(pair // 2 + int(rs.randint(2))) % 2])


def fin_cases():
    return [fin_case(s) for s in range(N_FIN)]


def fin_inputs(cfg):
    """Column sums of integer data in [-8, 8] (plus a per-column integer offset), exact in f32: summation error does not enter.
    Column 0 is constant.  -> (stats f32 [2, C], running_mean f32 [C], running_var f32 [C])"""
    rows, C = cfg["rows"], cfg["C"]
    g = torch.Generator().manual_seed(cfg["seed"])
    x = torch.randint(-8, 9, (rows, C), generator=g).double() + (torch.arange(C) % 5 - 2).double() * 3.0
    x[:, 0] = FIN_CONST_VALUE
    stats = torch.stack([x.sum(0), (x * x).sum(0)])
    assert float(stats.abs().max()) < 2.0 ** 24
    rm = torch.randn((C,), generator=g) * 2.0
    rv = torch.rand((C,), generator=g) * 3.0 + 0.5
    return stats.float(), rm, rv


def fin_reference(stats, rm, rv, cfg):
    """The BatchNorm formulas in fp64 on the f32 sums and the f32-rounded scalars the kernel receives: biased variance for rstd;
    the running update takes the UNBIASED variance, var * rows / (rows - 1), and for rows == 1 the kernel's factor of 1
    (nn.BatchNorm2d refuses a single value per channel in train(); the kernel defines it as the biased variance, 0).
    -> dict of fp64: mean, e2, var, rstd, run_mean, run_var (the last two None without running buffers)"""
    rows, eps, mom = float(cfg["rows"]), f32r(cfg["eps"]), f32r(cfg["momentum"])
    s, q = stats[0].double(), stats[1].double()
    mean, e2 = s / rows, q / rows
    var = torch.clamp(e2 - mean * mean, min=0.0)            # never negative in exact arithmetic; the clamp only removes fp64 dust
    out = dict(mean=mean, e2=e2, var=var, rstd=1.0 / torch.sqrt(var + eps), run_mean=None, run_var=None)
    if cfg["running"]:
        unbias = rows / (rows - 1.0) if rows > 1 else 1.0
        out["run_mean"] = (1.0 - mom) * rm.double() + mom * mean
        out["run_var"] = (1.0 - mom) * rv.double() + mom * var * unbias
    return out


def var_bound_finalize(e2, mean):
    """|error| of var = fl(fl(q / rows) - fl(m * m)), m = fl(s / rows), from exact s and q: the quotient q / rows rounds once
    (2^-24 E[x^2]), m carries one rounding which the product doubles and rounds again (3 x 2^-24 mean^2), and the difference rounds
    once (2^-24 var <= 2^-24 E[x^2]).  The clamp at 0 moves the result towards the true variance, which is never negative."""
    return SLACK * U32 * (2.0 * e2 + 3.0 * mean * mean)


def rstd_interval(var, dvar, eps):
    """rstd = fl(1 / fl(sqrt(fl(var' + eps)))) with |var' - var| <= dvar and var' >= 0 (the kernel clamps): the interval of the
    exact function over that range, widened by the three roundings (the sum's enters through the square root at half weight)."""
    lo = 1.0 / torch.sqrt(var + dvar + eps) * (1.0 - 3.0 * U32)
    hi = 1.0 / torch.sqrt(torch.clamp(var - dvar, min=0.0) + eps) * (1.0 + 3.0 * U32)
    return lo, hi


def interval_ratio(got, ref, lo, hi):
    """worst (got - ref) / (the interval's half on that side); <= 1 inside"""
    g = got.double()
    up_, dn = (g - ref) / (hi - ref + 1e-300), (ref - g) / (ref - lo + 1e-300)
    r = torch.where(g >= ref, up_, dn)
    return bool(torch.isfinite(g).all()) and bool((r <= 1.0).all()), float(r.max())


def fin_bounds(ref, rm, rv, cfg):
    """-> dict: mean (bound), rstd (lo, hi), run_mean, run_var (bounds).
    mean: one division.  running mean: fl(1 - momentum), its product with the old value, momentum * m, the sum: at most four
    roundings on either term.  running var: the same on the old value; momentum * var' * fl(rows / (rows - 1)) carries var's error
    and four roundings (the factor's division, two products, the sum)."""
    rows, mom = float(cfg["rows"]), f32r(cfg["momentum"])
    dvar = var_bound_finalize(ref["e2"], ref["mean"])
    out = dict(mean=SLACK * U32 * ref["mean"].abs(), rstd=rstd_interval(ref["var"], dvar, f32r(cfg["eps"])), dvar=dvar)
    if cfg["running"]:
        unbias = rows / (rows - 1.0) if rows > 1 else 1.0
        old_m, old_v = ((1.0 - mom) * rm.double()).abs(), ((1.0 - mom) * rv.double()).abs()
        out["run_mean"] = SLACK * U32 * (4.0 * old_m + 4.0 * (mom * ref["mean"]).abs())
        out["run_var"] = SLACK * (U32 * (4.0 * old_v + 5.0 * mom * unbias * ref["var"]) + mom * unbias * dvar)
    return out


def fin_restated(stats, rm, rv, cfg, defect=None):
    """bn_finalize_kernel in numpy f32.  defect: None, "biased_running_var", "momentum_on_old", "eps_outside_sqrt".
    -> (mean, rstd, run_mean or None, run_var or None) f32 tensors"""
    f = np.float32
    rows, eps, mom, one = f(cfg["rows"]), f(cfg["eps"]), f(cfg["momentum"]), f(1.0)
    s, q = stats[0].numpy(), stats[1].numpy()
    m = s / rows
    var = np.maximum(q / rows - m * m, f(0.0))
    rstd = one / (np.sqrt(var) + eps) if defect == "eps_outside_sqrt" else one / np.sqrt(var + eps)
    out = [torch.from_numpy(m), torch.from_numpy(rstd.astype(np.float32)), None, None]
    if cfg["running"]:
        unbias = one if defect == "biased_running_var" else rows / np.maximum(rows - one, one)
        a, b = (mom, one - mom) if defect == "momentum_on_old" else (one - mom, mom)
        out[2] = torch.from_numpy((a * rm.numpy() + b * m).astype(np.float32))
        out[3] = torch.from_numpy((a * rv.numpy() + b * var * unbias).astype(np.float32))
    return tuple(out)


# =====================================================================================================================
# mv_bn_act
# =====================================================================================================================
ACT_BODIES = ((BF16, BF16), (F32, BF16), (F32, F32))       # (x, y): the three kernel instances; the residual is in y's encoding
ACT_SHAPES = tuple((r, c) for r in (1, 3, 1000) for c in (4, 64, 68))
N_ACT = len(ACT_BODIES) * 4 * 3


def act_branches(cfg):
    body = "act_%s_to_%s" % (cfg["xdt"], cfg["ydt"])
    b = [body, body + ("+res" if cfg["res"] else "-res") + ("+relu" if cfg["relu"] else "-relu")]
    b.append("act_second_trip" if cfg["rows"] * (cfg["C"] // 4) > ONE_TRIP else "act_one_trip")
    return b


def act_case(seed):
    combo, rep = seed % 12, seed // 12
    xdt, ydt = ACT_BODIES[combo // 4]
    rows, C = ACT_SHAPES[(combo * 3 + rep * 4 + combo // 4) % len(ACT_SHAPES)]
    return dict(fam="act", seed=seed, xdt=xdt, ydt=ydt, res=bool(combo & 1), relu=bool(combo & 2), rows=rows, C=C)


ACT_FIXED = [
    # just past the grid cap: 4,194,400 rows of one channel group
    dict(fam="act", seed=8941, xdt=F32, ydt=BF16, res=True, relu=True, rows=ONE_TRIP + 96, C=4),
]


def act_cases():
    return [act_case(s) for s in range(N_ACT)] + ACT_FIXED


def act_inputs(cfg):
    """x [rows, C] (its encoding) spread around per-column means of a few units, so that x - mean cancels; rstd positive, gamma of
    both signs, beta; the residual [rows, C] in y's encoding.  About half of the pre-activations are negative."""
    rows, C = cfg["rows"], cfg["C"]
    g = torch.Generator().manual_seed(cfg["seed"])
    mean = torch.randn((C,), generator=g) * 4.0
    rstd = torch.rand((C,), generator=g) * 2.0 + 0.25
    gamma = (torch.rand((C,), generator=g) + 0.25) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    beta = torch.randn((C,), generator=g) * 0.3
    x = (mean + torch.randn((rows, C), generator=g) / rstd).to(DT[cfg["xdt"]])
    res = torch.randn((rows, C), generator=g).to(DT[cfg["ydt"]]) if cfg["res"] else None
    return x, mean, rstd, gamma, beta, res


def act_reference(x, mean, rstd, gamma, beta, res, cfg):
    """-> (y fp64, bound fp64), per element.  The kernel's f32 arithmetic: the difference, two products, the sum with beta, the sum
    with the residual -- a rounding each, so t = |(x - mean) rstd gamma| collects five, beta two, the residual one (a fused
    multiply-add only drops one).  A bf16 output adds half an ulp of bf16 at the magnitude the f32 result can have."""
    t = (x.double() - mean.double()) * rstd.double() * gamma.double()
    y = t + beta.double()
    bound = 5.0 * t.abs() + 2.0 * beta.double().abs()
    if res is not None:
        y = y + res.double()
        bound = bound + res.double().abs()
    bound = SLACK * U32 * bound
    if cfg["relu"]:
        y = torch.clamp(y, min=0.0)
    if cfg["ydt"] == BF16:
        bound = bound + half_ulp_bf16(y.abs() + bound)
    return y, bound


def act_restated(x, mean, rstd, gamma, beta, res, cfg, defect=None):
    """bn_act_kernel in torch f32, unfused.  defect: None, "residual_after_relu", "x_rounded_to_bf16_first"."""
    v = x.float()
    if defect == "x_rounded_to_bf16_first":
        v = v.to(torch.bfloat16).float()
    o = (v - mean) * rstd * gamma + beta
    if res is not None and defect != "residual_after_relu":
        o = o + res.float()
    if cfg["relu"]:
        o = torch.clamp(o, min=0.0)
    if res is not None and defect == "residual_after_relu":
        o = o + res.float()
    return o.to(DT[cfg["ydt"]])


# =====================================================================================================================
# variance conditioning of the single-pass batch statistics
# =====================================================================================================================
COND_ROWS, COND_C, COND_EPS = 12544, 64, 1e-5
COND_MU = (0.0, 1.0, 3.0, 10.0, 30.0, 100.0)
COND_CONST_VALUE = 3.7


def cond_inputs():
    """f32 [12544, 64]: column c is N(mu, 1) with mu = COND_MU[c % 6]; the last column is constant (3.7 rounded to f32, so its
    sums are not exact).  -> (x, mu per column (nan for the constant one))"""
    g = torch.Generator().manual_seed(1234)
    mu = torch.tensor(COND_MU)[torch.arange(COND_C) % len(COND_MU)]
    x = torch.randn((COND_ROWS, COND_C), generator=g) + mu
    x[:, -1] = COND_CONST_VALUE
    mu[-1] = NAN
    return x, mu


def cond_reference(x):
    """two-pass mean, biased variance and rstd in fp64, and the bounds of the single-pass formula var = E[x^2] - mean^2 on f32 sums:
    |dvar| <= 2 rows 2^-24 (E[x^2] + mean^2) + the finalize terms (var_bound_finalize); the mean carries the summation bound of its
    sum and the division's rounding; rstd the interval that dvar leaves it (rstd_interval, which knows the clamp at 0)."""
    v = x.double()
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    e2, e1 = (v * v).mean(0), v.abs().mean(0)
    dmean = 2.0 * COND_ROWS * U32 * e1 + U32 * mean.abs()
    dvar = 2.0 * COND_ROWS * U32 * (e2 + mean * mean) + var_bound_finalize(e2, mean)
    eps = f32r(COND_EPS)
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), dmean=dmean * SLACK, dvar=dvar, rstd_iv=rstd_interval(var, dvar, eps))


def cond_torch_f32(x):
    """what F.batch_norm in f32 on the CPU takes as the batch statistics of the same input (read back through running buffers with
    momentum 1; its unbiased variance converted back in fp64).  -> (mean, rstd) fp64"""
    C = x.shape[1]
    rm, rv = torch.zeros(C), torch.ones(C)
    F.batch_norm(x.float().cpu(), rm, rv, None, None, True, 1.0, COND_EPS)
    var = rv.double() * (COND_ROWS - 1.0) / COND_ROWS
    return rm.double(), 1.0 / torch.sqrt(var + f32r(COND_EPS))


# =====================================================================================================================
# census
# =====================================================================================================================
FAMILIES = {
    "nhwc": (nhwc_cases, nhwc_branches),
    "im2col": (im2col_cases, im2col_branches),
    "pool": (pool_cases, pool_branches),
    "stats": (stats_cases, stats_branches),
    "fin": (fin_cases, fin_branches),
    "act": (act_cases, act_branches),
}


def case_id(cfg):
    skip = ("fam", "seed")
    return "%s%d-" % (cfg["fam"], cfg["seed"]) + "-".join("%s%s" % (k, v) for k, v in cfg.items() if k not in skip)


def census(fam):
    """branch name -> number of cases of the family that reach it"""
    cases, branches = FAMILIES[fam]
    count = {}
    for c in cases():
        for b in branches(c):
            count[b] = count.get(b, 0) + 1
    return count
