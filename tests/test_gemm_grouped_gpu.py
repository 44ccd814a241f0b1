"""The grouped weight-gradient launch (mv_gemm_grouped_tn) on the GPU: many dW = dy^T.x products in one persistent launch, against fp64
products of the same 16-bit inputs, and the training step with the full-row layers' weight gradients grouped against the per-layer path.

Tolerance of the kernel tests: the one tests/test_kernels_gpu.py holds a full-K TN product to -- max |c - ref| < 2e-5 * sqrt(K) * max |ref|
(test_gemm_auto_dispatch_large, line 223; element-wise as in test_gemm_persistent_many_units_per_block, lines 259-263)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import medvill_amd as mv                                   # noqa: E402
from medvill_amd import hip_ops as ops                      # noqa: E402

DEV = "cuda"
# (No, Ko, rows): whole tiles, several tiles, a ragged problem whose rows are no multiple of 64.  7 tiles of 256 x 256 in all.
SHAPES = [(256, 256, 320), (512, 256, 448), (768, 256, 448), (200, 136, 333)]


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def make_problems(dt, shapes=SHAPES, seed=0):
    """Operands as the engine holds them: A a column slice of a buffer three times as wide (dqkv is), B and C with padded leading dimensions."""
    out = []
    for i, (No, Ko, rows) in enumerate(shapes):
        lda, ldb, ldc = 3 * No, Ko + 8, Ko + 4
        abuf, bbuf = rnd((rows, lda), dt, seed + 10 * i + 1, 0.5), rnd((rows, ldb), dt, seed + 10 * i + 2, 0.5)
        a, b = abuf[:, No:2 * No], bbuf[:, :Ko]
        c = torch.full((No, ldc), 0.25, dtype=torch.float32, device=DEV)
        out.append((a, b, c, No, Ko, rows, lda, ldb, ldc))
    return out


_REF = {}


def reference(dt, shapes=SHAPES, seed=0):
    key = (dt, tuple(shapes), seed)
    if key not in _REF:
        _REF[key] = [(a.double().t() @ b.double()) for a, b, *_ in make_problems(dt, shapes, seed)]
    return _REF[key]


def check(problems, refs, alpha=None, accumulate=False):
    for (a, b, c, No, Ko, rows, lda, ldb, ldc), ref in zip(problems, refs):
        want = ref * (float(alpha) if alpha is not None else 1.0) + (0.25 if accumulate else 0.0)
        err = (c[:, :Ko].double() - want).abs().max()
        print(f"grouped dW {No}x{Ko} over {rows}: max err {float(err):.3e} of scale {float(want.abs().max()):.3e}")
        assert float(err) < 2e-5 * math.sqrt(rows) * float(want.abs().max())
        assert torch.all(c[:, Ko:] == 0.25)                      # nothing is written past a row's Ko columns


def run(problems, dt, blocks, alpha=None, accumulate=False, table=None):
    ops.set_persistent_cus(blocks)
    try:
        t = table or ops.GroupedTN(DEV)
        t.set(dt, problems)
        wb = t.workspace_bytes()
        ws = torch.empty(max(wb // 4, 1), dtype=torch.float32, device=DEV)
        t.launch(ws=ws if wb else None, accumulate=accumulate, alpha=alpha)
        torch.cuda.synchronize()
        return t
    finally:
        ops.set_persistent_cus(0)


# blocks -> what the 7 units become: 0 (one block per CU) fewer units than blocks, all unsplit; 3: two rounds + one tile cut 3 ways;
# 5: one round + two tiles cut in halves; 4: one round + three unsplit units (75 % of a round); 7: exactly one round
@pytest.mark.parametrize("blocks,plan", [(0, (7, 0, 1)), (3, (6, 1, 3)), (5, (5, 2, 2)), (4, (7, 0, 1)), (7, (7, 0, 1))])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_grouped_products_match_fp64(dt, blocks, plan):
    problems = make_problems(dt)
    t = run(problems, dt, blocks)
    hdr = torch.frombuffer(t.host, dtype=torch.int32, count=16).tolist()
    assert tuple(hdr[5:8]) == plan
    assert (t.workspace_bytes() > 0) == (plan[2] > 1)
    check(problems, reference(dt))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("use_alpha", [False, True])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_alpha_and_accumulate_on_unsplit_and_split_units(dt, use_alpha, accumulate):
    alpha = torch.tensor([1.0 / 1024.0], dtype=torch.float32, device=DEV) if use_alpha else None
    problems = make_problems(dt)
    run(problems, dt, 3, alpha=alpha, accumulate=accumulate)          # 6 unsplit units and a tile in 3 slices
    check(problems, reference(dt), alpha=alpha, accumulate=accumulate)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_one_problem_equals_mv_gemm_bit_for_bit(dt):
    alpha = torch.tensor([1.0 / 64.0], dtype=torch.float32, device=DEV)
    for i, prob in enumerate(make_problems(dt)):
        a, b, c, No, Ko, rows, lda, ldb, ldc = prob
        for al, acc in ((None, False), (alpha, True)):
            c.fill_(0.25)
            t = run([prob], dt, 0, alpha=al, accumulate=acc)
            assert torch.frombuffer(t.host, dtype=torch.int32, count=16).tolist()[7] == 1          # nothing splits
            c1 = torch.full_like(c, 0.25)
            ops.gemm(a, b, c1, ta=True, tb=True, M=No, N=Ko, K=rows, lda=lda, ldb=ldb, ldc=ldc, splitk=1, alpha=al, accumulate=acc)
            assert torch.equal(c, c1), i


def test_short_contraction_in_the_tail_and_a_refilled_table():
    dt = torch.bfloat16
    shapes = SHAPES + [(128, 64, 100)]                          # 8 units on 7 blocks: the last tile in 5 slices, three of them empty
    problems = make_problems(dt, shapes, seed=100)
    t = run(problems, dt, 7)
    assert torch.frombuffer(t.host, dtype=torch.int32, count=16).tolist()[5:8] == [7, 1, 5] and t.uploads == 1
    check(problems, reference(dt, shapes, seed=100))
    # the same table object, other problems (pointers, shapes and count change): rebuilt once, then reused
    problems2 = make_problems(dt)
    run(problems2, dt, 3, table=t)
    assert t.uploads == 2
    check(problems2, reference(dt))
    for _, _, c, *_ in problems2:
        c.fill_(0.25)
    run(problems2, dt, 3, table=t)
    assert t.uploads == 2 and t.launches == 3                   # nothing changed: no copy
    check(problems2, reference(dt))


def test_launch_rejects_leave_the_outputs_alone():
    dt = torch.bfloat16
    problems = make_problems(dt)
    ops.set_persistent_cus(3)
    try:
        t = ops.GroupedTN(DEV)
        t.set(dt, problems)
        with pytest.raises(RuntimeError, match="MV_E_WORKSPACE"):
            t.launch(ws=None)
        with pytest.raises(RuntimeError, match="MV_E_WORKSPACE"):
            t.launch(ws=torch.empty(16, dtype=torch.float32, device=DEV))
        bad = list(problems)
        bad[2] = (problems[2][0][:, 4:], *problems[2][1:])       # A 8 bytes off a 16-byte boundary
        with pytest.raises(RuntimeError, match="MV_E_SHAPE"):
            ops.GroupedTN(DEV).set(dt, bad)
    finally:
        ops.set_persistent_cus(0)
    torch.cuda.synchronize()
    assert all(torch.all(c == 0.25) for _, _, c, *_ in problems)


# ------------------------------------------------------------------------------------------ the training step
def _step(monkeypatch, grouped, hook=False, parts=1):
    monkeypatch.setenv("MV_GROUPED_DW", "1" if grouped else "0")
    monkeypatch.setenv("MV_GROUPED_DW_PARTS", str(parts))
    cfg = mv.ModelConfig(hidden=128, heads=2, intermediate=512, layers=3, vocab_size=1024, max_pos=512, dropout=0.1)
    B, N, S = 4, 6, 56                                          # L = N + S + 2 = 64
    b = mv.data.synthetic_batch(cfg.vocab_size, B, N, S, "full", seed=41, device=DEV, lengths=[56, 17, 40, 3])
    torch.manual_seed(77)
    model = mv.CXRBERT(cfg, None, dtype=torch.bfloat16, device=DEV)
    model.reset_parameters(seed=6)
    model.train()
    eng = model.engine
    assert eng.grouped_dw == grouped
    calls = []
    if hook:
        orig = eng.encoder_backward
        eng.encoder_backward = lambda bucket_hook=None: orig(bucket_hook=lambda name, ev: calls.append(name))
    ts = mv.TrainStep(model, lr=0.0)
    stats = ts(dict(b), train=True).cpu()
    torch.cuda.synchronize()
    assert eng.S["cu"] is not None and eng.S["p_drop"] == pytest.approx(0.1)           # packed (ragged) rows, dropout on
    launches = sum(t.launches for t in eng._dw_group.values())
    _step.full_layers = sum(1 for a in eng.S["layers"] if a["rows"] == eng.S["M"])        # layers whose backward ran on every row
    return stats, {k: v.clone() for k, v in eng.g.items()}, launches, calls


def same_loss(sa, sb):
    """The forward and the heads run the same kernels on the same data in both runs: label / sample counts and correct predictions are
    equal, and the two loss sums are equal up to the order of the f32 atomic adds that form them (a few ulp of a sum of <= 20 terms).
    This departs from the wording the test was specified with ("the losses must be equal"): the MLM and ITM loss sums are formed with
    f32 atomicAdd (mv_rowops.hip, the loss kernels), so two runs of the SAME path already differ in the last bits; 4 ulp of the sum
    is the bound for reordering <= 20 positive terms, and the integer counts beside them are compared exactly."""
    assert torch.equal(sa[[1, 2, 4, 5]], sb[[1, 2, 4, 5]])
    for i in (0, 3):
        assert abs(float(sa[i]) - float(sb[i])) <= 4 * 1.2e-7 * abs(float(sa[i])), (i, float(sa[i]), float(sb[i]))


def test_training_step_with_grouped_weight_gradients_equals_the_per_layer_path(monkeypatch):
    s1, g1, n1, _ = _step(monkeypatch, True, parts=0)           # the default: two full-row layers per launch
    assert _step.full_layers >= 2 and n1 == (_step.full_layers + 1) // 2
    s0, g0, n0, _ = _step(monkeypatch, False)
    assert n0 == 0
    s4, g4, n4, _ = _step(monkeypatch, True, parts=1)           # all of them in one launch
    assert n4 == 1
    same_loss(s4, s0)
    for k in g0:
        assert float((g4[k] - g0[k]).norm()) <= 3e-3 * float(g0[k].norm()), k
    same_loss(s0, s1)
    # tests/test_model_gpu.py:306 holds packed against padded gradients to |g0 - g1| / |g0| < 3e-3; here per parameter tensor
    worst = 0.0
    for k in g0:
        d, n = float((g0[k] - g1[k]).norm()), float(g0[k].norm())
        worst = max(worst, d / max(n, 1e-30))
        assert d <= 3e-3 * n, (k, d, n)
    print(f"grouped vs per-layer weight gradients: worst relative difference {worst:.2e}")
    # MV_GROUPED_DW_PARTS=2: two launches
    s3, g3, n3, _ = _step(monkeypatch, True, parts=2)
    assert n3 == 2
    same_loss(s3, s0)
    for k in g0:
        assert float((g3[k] - g0[k]).norm()) <= 3e-3 * float(g0[k].norm()), k
    # under a bucket hook (data parallel) the per-layer path runs whatever the switch says
    s2, g2, n2, calls = _step(monkeypatch, True, hook=True)
    assert n2 == 0 and calls[0] == "heads" and calls[-1] == "embeddings" and "layer0" in calls
    same_loss(s2, s0)
    for k in g0:                                                # (not bit for bit: LayerNorm / bias gradients are sums of atomics)
        assert float((g2[k] - g0[k]).norm()) <= 3e-3 * float(g0[k].norm()), k
