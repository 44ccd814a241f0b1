"""Branch census and self-checks of the embedding sweep (CPU).  tests/test_wave_per_row_embed_sweep_gpu.py is only worth its GPU time
while its cases reach what the fixed-shape tests of embed_fwd_kernel / embed_bwd_kernel never take; this file counts those branches, pins the constants
the predicates rely on to the source, checks the generator against the ABI, checks the fp64 reference against a second formulation,
runs every bound of the sweep on a plain f32 torch implementation (no kernel anywhere), and holds the truth table of emb_decode."""
import ast
import os
import re

import numpy as np
import pytest
import torch

import embed_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modality-self-supervision_amd", "csrc")
HIP = os.path.join(CSRC, "mv_rowops.hip")
GPU_FILE = os.path.join(ROOT, "tests", "test_wave_per_row_embed_sweep_gpu.py")
MIN_HITS = 3

# everything the sweep exists for, by the names embed_cases.emb_branches gives
REQUIRED = ["nc1", "nc3", "nc4", "nc8", "ragged_chunk", "dt_f32", "dt_bf16", "dt_f16", "x0_bf16", "rowmap_none", "rowmap_prefix", "rowmap_perm",
            "n_rows%4=0", "n_rows%4=1", "n_rows%4=2", "n_rows%4=3", "bwd_row_walk", "img_pos_none", "N=0", "drop_0_0", "drop_0.1_0.1",
            "drop_0.1_0.5", "unscale_none", "unscale_0.25", "unscale_0.000976562", "pad_0", "pad_-1", "pad_103", "hot>=V", "hot==V-1",
            "hot_rows", "bad_tok_high", "bad_tok_neg1", "bad_tok_below_neg1", "bad_pos", "bad_seg"]


def test_every_named_branch_is_reached():
    count = C.emb_census()
    print(f"\nemb: {len(C.emb_cases())} cases")
    for name in sorted(set(REQUIRED) | set(count)):
        print(f"    {name:32s} {count.get(name, 0):4d}{'' if name in REQUIRED else '   (not required)'}")
    short = {n: count.get(n, 0) for n in REQUIRED if count.get(n, 0) < MIN_HITS}
    assert not short, f"branches reached fewer than {MIN_HITS} times: {short}"


def test_the_value_sets_are_all_drawn():
    cases = C.emb_cases()

    def seen(key):
        return {c[key] for c in cases}
    assert seen("H") == set(C.EMB_H) and seen("dt") == {C.F32, C.BF16, C.F16} and seen("eps") == set(C.EMB_EPS)
    assert {(c["B"], c["N"], c["T"]) for c in cases} >= set(C.EMB_SHAPES)
    assert {(c["p_drop"], c["p_drop_img"]) for c in cases} == set(C.EMB_DROP)
    assert seen("unscale") == set(C.EMB_UNSCALE) and seen("pad") == set(C.EMB_PAD) and seen("V") == set(C.EMB_V)
    assert seen("rowmap") == set(C.EMB_ROWMAPS) and len(cases) >= 64
    # the text of most cases carries repeated ids, pad ids and a run of id 103
    rich = 0
    for c in cases:
        txt = C.emb_ids(c)["txt"]
        pad = c["pad"] if c["pad"] >= 0 else 0
        rich += bool((txt == C.EMB_HOT_TOKEN).sum() >= 2 and (txt == pad).any() and len(np.unique(txt)) < txt.size)
    assert 2 * rich > len(cases), rich
    # BERT-base's own row: H = 768 in bf16 over packed rows with dropout and unscale
    assert any(c["H"] == 768 and c["dt"] == C.BF16 and c["rowmap"] != "none" and c["p_drop"] > 0 and c["unscale"] is not None for c in cases)
    walk = [c for c in cases if "bwd_row_walk" in C.emb_branches(c)]
    assert any(c["rowmap"] == "none" and c["H"] <= 132 for c in walk) and any(c["rowmap"] != "none" and c["H"] <= 132 for c in walk)


def test_generated_cases_are_inside_the_abi():
    """A generator that draws what the launchers reject, or an id that could take an unfixed kernel outside its buffers, is a bug in the
    generator: the GPU file has no way to drop a case."""
    for c in C.emb_cases():
        B, N, T, L = c["B"], c["N"], c["T"], C.emb_L(c)
        assert c["H"] % 4 == 0 and 0 < c["H"] <= C.EMB_MAX_H and B > 0 and N >= 0 and T > 0 and c["V"] > 0, c
        assert T <= c["maxpos"], c
        assert not c["x0_bf16"] or c["dt"] == C.F16, c
        assert not (c["img_pos"] and N == 0), c
        rm = C.emb_rowmap(c)
        if rm is not None:
            assert rm.dtype == np.int32 and 0 < len(rm) <= B * L and len(set(rm.tolist())) == len(rm) and rm.min() >= 0 and rm.max() < B * L, c
        if c["rowmap"] == "prefix":
            assert bool((np.diff(rm) > 0).all()), c
            for b in range(B):                               # per sample the positions 0..len-1
                mine = rm[(rm // L) == b] - b * L
                assert len(mine) >= 1 and np.array_equal(mine, np.arange(len(mine))), c
        ids = C.emb_ids(c)
        assert ids["cls"].shape == (B,) and ids["sep"].shape == (B,) and ids["txt"].shape == (B, T) and ids["seg"].shape == (B, T), c
        assert (ids["img_pos"] is None) == (not c["img_pos"]) and (ids["img_pos"] is None or ids["img_pos"].shape == (B, N)), c
        # negative token ids: samples b >= 1 of cases with N >= 1 only
        neg_b = set(np.flatnonzero(ids["cls"] < 0)) | set(np.flatnonzero(ids["sep"] < 0)) | set(np.flatnonzero((ids["txt"] < 0).any(axis=1)))
        assert not neg_b or (N >= 1 and min(neg_b) >= 1), (c, neg_b)
        inp = C.emb_inputs(c)
        assert inp["n_rows"] == C.emb_n_rows(c) and inp["dx0"].shape == (inp["n_rows"], c["H"]) and (inp["imgproj"] is None) == (N == 0), c
        assert all(float((v != 0).float().mean()) > 0.99 for v in inp["prev"].values()), c      # a previous gradient, not a zeroed buffer


def test_the_gpu_file_cannot_drop_a_case():
    src = open(GPU_FILE).read()
    for node in ast.walk(ast.parse(src)):
        assert not isinstance(node, (ast.Continue, ast.Break)), f"line {node.lineno}: a loop over cases or checks must run to its end"
        if isinstance(node, ast.Attribute):
            assert node.attr not in ("skip", "skipif", "xfail", "importorskip", "exit"), f"line {node.lineno}: {node.attr}"
    assert re.search(r'parametrize\("cfg", C\.emb_cases\(\)', src)


def test_the_constants_in_the_source_are_the_constants_of_the_predicates():
    src = open(HIP).read()
    disp = open(os.path.join(CSRC, "mv_dispatch.h")).read()

    def body(name):
        i = src.index('extern "C" int %s(' % name)
        return src[i:src.find("\n}\n", i)]

    def num(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert num(src, r"#define MV_MAX_H (\d+)") == C.EMB_MAX_H == 2048
    m = re.search(r"mv_with_row_chunks\(int H,.*?H <= (\d+)\) return f\(std::integral_constant<int, 1>.*?H <= (\d+)\) return f\(std::integral_constant<int, 3>"
                  r".*?H <= (\d+)\) return f\(std::integral_constant<int, 4>.*?return f\(std::integral_constant<int, 8>", disp, re.S)
    assert m and tuple(int(x) for x in m.groups()) == C.EMB_NC_STEPS == (256, 768, 1024)
    assert num(src, r"#define MV_HOT_TOKEN (\d+)") == C.EMB_HOT_TOKEN == 103
    fwd, bwd = body("mv_embed_fwd"), body("mv_embed_bwd")
    assert num(bwd, r"if \(blocks > (\d+)\) blocks = \1;") == C.EMB_BWD_BLOCKS == 1024
    assert num(fwd, r"grid\(\(a\.n_rows \+ 3\) / (\d+)\)") == C.EMB_ROWS_PER_BLOCK == 4
    assert num(bwd, r"blocks = \(a\.n_rows \+ 3\) / (\d+);") == C.EMB_ROWS_PER_BLOCK
    assert "mv_with_row_chunks(H," in fwd and "mv_with_row_chunks(H," in bwd and "MV_HOT_TOKEN" in bwd
    for k in ("embed_fwd_kernel", "embed_bwd_kernel"):       # four waves of 64 lanes: one row each
        assert re.search(r"__launch_bounds__\(256\) void %s\(" % k, src), k
    assert re.search(r"embed_bwd_kernel.*?row = blockIdx\.x \* 4 \+ wl; row < M; row \+= gridDim\.x \* 4", src, re.S)
    # sizes derived from the caps
    walk = [c for c in C.emb_cases() if C.emb_n_rows(c) > C.EMB_BWD_BLOCKS * C.EMB_ROWS_PER_BLOCK]
    assert len(walk) >= MIN_HITS and all(C.emb_n_rows(c) <= CPU_MAX_ROWS for c in C.emb_cases() if c not in walk)


# ---- emb_decode --------------------------------------------------------------------------------------------------------------------
def test_decode_truth_table():
    """(l, id) -> (tok, pos, typ, reg) of emb_decode, id by id: B = 2, N = 2, T = 3, V = 50, maxpos = 8 (L = 7)."""
    cfg = dict(B=2, N=2, T=3, V=50, maxpos=8)
    I = 2 ** 31

    def dec(l, tok=7, seg=0, ipos=(3, 4), with_pos=True, b=1):
        ids = dict(cls=np.array([11, tok]), sep=np.array([12, tok]), txt=np.full((2, 3), tok), seg=np.full((2, 3), seg),
                   img_pos=np.array([[0, 1], list(ipos)]) if with_pos else None)
        t, p, ty, r, bb = C.emb_decode_host(cfg, ids, [b * 7 + l])
        assert int(bb[0]) == b
        return int(t[0]), int(p[0]), int(ty[0]), int(r[0])
    # token positions: [CLS] l = 0, [SEP] l = N + 1 = 3, text l = 4..6 (position l - 4, its own segment)
    for tok, want in ((7, 7), (0, 0), (49, 49), (50, 49), (57, 49), (I - 1, 49), (-1, 0), (-5, 0), (-I, 0), (103, 49)):
        assert dec(0, tok) == (want, 0, 0, -1), tok
        assert dec(3, tok) == (want, 0, 0, -1), tok
        assert dec(4, tok, seg=1) == (want, 0, 1, -1), tok
        assert dec(6, tok, seg=0) == (want, 2, 0, -1), tok
    for seg, want in ((0, 0), (1, 1), (-1, 0), (2, 1), (7, 1), (-I, 0)):
        assert dec(5, 7, seg=seg) == (7, 1, want, -1), seg
    # image rows l = 1..N: tok -1, the region, type 0, the clamped position -- whatever the token arrays hold
    for ipos, want in ((3, 3), (0, 0), (7, 7), (-3, 0), (8, 7), (17, 7)):
        assert dec(1, tok=-1, seg=7, ipos=(ipos, 4)) == (-1, want, 0, 0), ipos
        assert dec(2, tok=-5, ipos=(4, ipos)) == (-1, want, 0, 1), ipos
    assert dec(1, with_pos=False) == (-1, -1, 0, 0) and dec(2, with_pos=False) == (-1, -1, 0, 1)       # no position embedding
    assert dec(0, with_pos=False) == (7, 0, 0, -1) and dec(6, with_pos=False) == (7, 2, 0, -1)
    # only l in 1..N is an image row: nowhere else does reg >= 0 or tok < 0 come out
    for tok in (-1, -2, -I):
        for l in (0, 3, 4, 5, 6):
            t, _, _, r = dec(l, tok)
            assert t == 0 and r == -1, (l, tok)
    # the sample index and N = 0
    assert dec(0, b=0) == (11, 0, 0, -1) and dec(3, b=0) == (12, 0, 0, -1)
    cfg0 = dict(B=1, N=0, T=1, V=50, maxpos=1)
    ids0 = dict(cls=np.array([-1]), sep=np.array([60]), txt=np.array([[5]]), seg=np.array([[1]]), img_pos=None)
    t, p, ty, r, _ = C.emb_decode_host(cfg0, ids0, [0, 1, 2])
    assert t.tolist() == [0, 49, 5] and p.tolist() == [0, 0, 0] and ty.tolist() == [0, 0, 1] and r.tolist() == [-1, -1, -1]
    assert C.c_int([2 ** 31 - 1, -2 ** 31, -1, 5]).tolist() == [2 ** 31 - 1, -2 ** 31, -1, 5]


def test_decode_in_the_source_clamps_negative_token_ids():
    """tok == -1 means "image region" to both kernels, which then index imgproj / dimg with reg: the source has to clamp EVERY negative id
    at a token position, -1 included, and only the l in 1..N branch may hand out tok = -1 and a region."""
    src = open(HIP).read()
    i = src.index("void emb_decode(")
    dec = src[i:src.index("\n}\n", i)]
    assert re.search(r"if \(tok >= a\.V\) tok = a\.V - 1;", dec)
    assert re.search(r"if \(reg < 0 && tok < 0\) tok = 0;", dec)
    assert not re.search(r"tok < -1", dec), "a clamp that lets -1 through"
    assert re.search(r"^\s*reg = -1;", dec, re.M) and len(re.findall(r"\breg = ", dec)) == 2 and len(re.findall(r"tok = -1;", dec)) == 1
    assert re.search(r"else if \(l <= a\.N\) \{\s*tok = -1; reg = l - 1;", dec)
    for k in ("embed_fwd_kernel", "embed_bwd_kernel"):       # what the two kernels do with a negative tok
        j = src.index("void %s(" % k)
        kernel = src[j:src.index("\n}\n", j)]
        assert "emb_decode(a, b, l, tok, pos, typ, reg);" in kernel
        assert re.search(r"\(\(size_t\)b \* a\.N \+ reg\) \* H", kernel), k


# ---- the reference against a second formulation (fp64 against fp64: 1e-12 relative) --------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


CPU_MAX_ROWS = 600          # the CPU runs take every case of at most this many rows (all but the three row-walk cases)
SMALL = [c for c in C.emb_cases() if C.emb_n_rows(c) <= CPU_MAX_ROWS]


@pytest.mark.parametrize("cfg", SMALL, ids=lambda c: str(c["seed"]))
def test_reference_equals_the_closed_form_with_index_add(cfg):
    inp = C.emb_inputs(cfg)
    ref = C.emb_reference(cfg, inp)
    alt = C.emb_reference_closed_form(cfg, inp, ref)
    names = ("pre", "dpre", "dE", "dP", "dTy", "dg", "db") + (("dimg",) if cfg["N"] else ())
    for name in names:
        assert _rel(ref[name], alt[name]) < 1e-12, (cfg, name, _rel(ref[name], alt[name]))
    # F.embedding(padding_idx): no look-up gradient for the pad row; with pad id -1 row 0 is an ordinary row
    if 0 <= cfg["pad"] < cfg["V"]:
        assert float(ref["dE"][cfg["pad"]].abs().max()) == 0.0
    text_tok = ref["tok"][~ref["is_img"]]
    if cfg["pad"] == -1 and bool((text_tok == 0).any()):
        assert float(ref["dE"][0].abs().max()) > 0.0
    assert bool((text_tok >= 0).all()) and bool((text_tok < cfg["V"]).all()) and bool((ref["tok"][ref["is_img"]] == -1).all())
    # the dropout: dropped elements are zero, the two kinds of row keep their own share
    assert bool((ref["x0"][~ref["keep"]] == 0).all())
    if cfg["p_drop_img"] == 0.5 and int(ref["is_img"].sum()) * cfg["H"] >= 20000:
        assert abs(float(ref["keep"][ref["is_img"]].double().mean()) - 0.5) < 0.02
        assert abs(float(ref["keep"][~ref["is_img"]].double().mean()) - 0.9) < 0.02


def test_the_cpu_cases_reach_every_branch_but_the_row_walk():
    names = set()
    for c in SMALL:
        names |= set(C.emb_branches(c))
    assert set(REQUIRED) - names == {"bwd_row_walk"}, set(REQUIRED) - names


# ---- the bounds, without any kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", SMALL, ids=lambda c: f"{c['seed']}-{c['dt']}-H{c['H']}-B{c['B']}")
def test_plain_f32_torch_passes_every_bound_of_the_sweep(cfg):
    """The bounds of check_forward / check_backward are derivations, not measurements of the kernels: a plain f32 torch implementation
    on the CPU (LayerNorm by hand, index_add_ for the tables) has to pass them all, on every case of at most CPU_MAX_ROWS rows."""
    inp = C.emb_inputs(cfg)
    ref = C.emb_reference(cfg, inp)
    fwd_tol, bwd_tol = C.emb_tolerances(cfg, inp, ref)
    fwd, bwd = C.emb_plain_f32(cfg, inp, ref)
    C.check_forward(cfg, inp, ref, fwd, fwd_tol)
    C.check_backward(cfg, inp, ref, bwd, bwd_tol)


def test_the_checks_notice_a_wrong_row():
    """one wrong packed row of x0, one wrong row of dE and a gradient on the pad row each fail the checks that passed before"""
    cfg = next(c for c in SMALL if c["seed"] == 9704)
    inp = C.emb_inputs(cfg)
    ref = C.emb_reference(cfg, inp)
    fwd_tol, bwd_tol = C.emb_tolerances(cfg, inp, ref)
    fwd, bwd = C.emb_plain_f32(cfg, inp, ref)
    bad = dict(fwd, x0=fwd["x0"].clone())
    bad["x0"][3] = fwd["x0"][4]
    with pytest.raises(AssertionError):
        C.check_forward(cfg, inp, ref, bad, fwd_tol)
    tok = int(ref["tok"][~ref["is_img"]].max())
    for row, scale in ((tok, 1.01), (cfg["pad"], 1.0 + 2.0 ** -20)):
        bad = dict(bwd, dE=bwd["dE"].clone())
        bad["dE"][row] *= scale
        with pytest.raises(AssertionError):
            C.check_backward(cfg, inp, ref, bad, bwd_tol)


NEG1 = [c for c in SMALL if "bad_tok_neg1" in C.emb_branches(c)]


@pytest.mark.parametrize("cfg", NEG1, ids=lambda c: str(c["seed"]))
def test_the_checks_notice_an_id_of_minus_one_taken_for_an_image_region(cfg):
    """What emb_decode did before it clamped -1 at token positions, written out on the plain f32 outputs: such a row read region
    b * N - 1 of imgproj instead of word 0, added nothing to dE, and stored its gradient over that region of dimg.  Forward and backward
    checks each fail on it, by value (the generator keeps such ids in samples b >= 1, so the region exists)."""
    N = cfg["N"]
    inp = C.emb_inputs(cfg)
    ref = C.emb_reference(cfg, inp)
    fwd_tol, bwd_tol = C.emb_tolerances(cfg, inp, ref)
    fwd, bwd = C.emb_plain_f32(cfg, inp, ref)
    li = np.arange(inp["n_rows"]) if inp["rowmap_np"] is None else inp["rowmap_np"]
    raw_tok, _, _, m_img, b = C.emb_raw_rows(cfg, inp["ids"], li)
    rows = np.flatnonzero(~m_img & (raw_tok == -1))
    assert len(rows) and b[rows].min() >= 1 and N >= 1
    region = torch.from_numpy(b[rows] * N - 1)
    rows = torch.from_numpy(rows)
    e_old, e_new = inp["imgproj"][region].float(), inp["E"][0].float()
    assert bool((e_old != e_new).any())
    # forward: the row sum built on the wrong source row -- pre alone, then x0 alone (LayerNorm of the wrong sum, undropped)
    pre_old = fwd["pre"][rows] - e_new + e_old
    bad = dict(fwd, pre=fwd["pre"].clone())
    bad["pre"][rows] = pre_old
    with pytest.raises(AssertionError, match="pre differs"):
        C.check_forward(cfg, inp, ref, bad, fwd_tol)
    y_old = torch.nn.functional.layer_norm(pre_old, (cfg["H"],), inp["gamma"], inp["beta"], cfg["eps"])
    bad = dict(fwd, x0=fwd["x0"].clone())
    bad["x0"][rows] = (y_old * ref["keep"][rows] * ref["scale"][rows].float()).to(fwd["x0"].dtype)
    with pytest.raises(AssertionError, match="x0"):
        C.check_forward(cfg, inp, ref, bad, fwd_tol)
    # backward: no look-up gradient from these rows (visible unless row 0 is the pad row), and their gradient stored into dimg
    us = 1.0 if cfg["unscale"] is None else cfg["unscale"]
    dpre = ref["dpre"][rows].float()
    if cfg["pad"] != 0:
        bad = dict(bwd, dE=bwd["dE"].clone())
        bad["dE"][0] -= us * dpre.sum(0)
        with pytest.raises(AssertionError, match="dE"):
            C.check_backward(cfg, inp, ref, bad, bwd_tol)
    bad = dict(bwd, dimg=bwd["dimg"].clone())
    bad["dimg"][region] = dpre.to(bwd["dimg"].dtype)
    with pytest.raises(AssertionError, match="dimg"):
        C.check_backward(cfg, inp, ref, bad, bwd_tol)
