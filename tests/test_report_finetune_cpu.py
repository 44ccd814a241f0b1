"""Report-generation fine-tuning, host logic (CPU only): the fp64 restatement against numbers recorded from the reference's own
LabelSmoothingLoss, the plan builder, the kept-sample count, the data helper, the export and the new C-ABI entries, the fine-tune
checkpoint layout and the optimizer's table of unreached tensors."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                                   # noqa: E402
from medvill_amd import _lib                               # noqa: E402
from medvill_amd.checkpoint import to_finetune_keys        # noqa: E402
from medvill_amd.report_finetune import build_plan, keep_count   # noqa: E402
import report_finetune_cases as C                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, max_position_embeddings=128)
NEW = ("mv_lm_loss_fwd", "mv_lm_loss_select", "mv_lm_loss_bwd")
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
P = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before a launch


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_matches_the_recorded_reference_numbers():
    g = np.load(os.path.join(ROOT, "tests", "golden", "report_finetune_loss.npz"))
    for name, shape in (("a", (5, 4, 37)), ("b", (2, 3, 300))):
        z, lab = torch.from_numpy(g[f"{name}_logits"]), torch.from_numpy(g[f"{name}_labels"])
        assert tuple(z.shape) == shape and int(lab.min()) == 0 and int(lab.max()) == shape[2] - 1
        for ls in (0.1, 1.0):
            want = torch.from_numpy(g[f"{name}_loss_{ls}"]).double()
            got = C.slot_loss(z, lab, ls)
            assert float((got - want).abs().max()) < 1e-7, (name, ls)
            assert bool((got[lab == 0] == 0).all()) and bool((got[lab != 0] > 0).all())


def test_closed_form_of_the_kernels_equals_the_restatement():
    """include/medvill.h states the smoothed loss as c log c + (V-2) s log s - c (z[t] - lse) - s ((zsum - z[t]) - (V-2) lse)."""
    g = torch.Generator().manual_seed(4)
    for V, ls in ((37, 0.1), (300, 1.0), (300, 0.3)):
        z = (torch.randn(6, V, generator=g) * 3).double()
        t = torch.tensor([1, 2, V - 1, 5, 7, 3])
        c, s = C.smoothing_constants(ls, V)
        lse = torch.logsumexp(z, -1)
        zt = z.gather(1, t.view(-1, 1)).view(-1)
        zsum = z[:, 1:].sum(-1)
        closed = (c * np.log(c) if c > 0 else 0.0) + (V - 2) * s * np.log(s) - c * (zt - lse) - s * ((zsum - zt) - (V - 2) * lse)
        assert float((closed - C.slot_loss(z, t, ls)).abs().max()) < 1e-9


@pytest.mark.parametrize("B,r,k", [(10, 0.9, 0), (64, 0.3, 44), (5, 0.2, 4), (8, 0.25, 6), (1, 0.2, 0), (4, 0.0, 4)])
def test_kept_sample_count_is_the_reference_expression(B, r, k):
    assert keep_count(B, r) == k == C.keep_count(B, r)


# ------------------------------------------------------------------------------------------------ plan builder
def test_plan_drops_zero_weights_and_keeps_duplicates():
    L, V = 20, 50
    pos = torch.tensor([[5, 5, 7, 0], [3, 3, 0, 0], [0, 0, 0, 0], [9, 4, 9, 6]])
    ids = torch.tensor([[11, 11, 12, 0], [21, 22, 0, 0], [0, 0, 0, 0], [31, 32, 33, 34]])
    w = torch.tensor([[1, 1, 0.5, 0], [1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0.0]])
    p = build_plan(pos, ids, w, L=L, V=V)
    assert p["B"] == 4 and p["U"] == 5 and p["n"] == 8
    assert p["rows"].tolist() == [5, 7, 23, 64, 69] and p["rows"].dtype == torch.int32          # sample 2 contributes nothing
    assert p["row_ptr"].tolist() == [0, 2, 3, 5, 6, 8]
    assert p["labels"].tolist() == [11, 11, 12, 21, 22, 32, 31, 33]                             # equal and different labels on one row
    assert p["sample"].tolist() == [0, 0, 0, 1, 1, 3, 3, 3]
    assert p["weights"].tolist() == [1, 1, 0.5, 1, 1, 1, 1, 1]
    empty = build_plan(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3), L=L, V=V)
    assert empty["U"] == 0 and empty["n"] == 0 and empty["row_ptr"].tolist() == [0]


def test_plan_refuses_what_the_kernels_cannot_take():
    one = lambda p, t, w=1.0: (torch.tensor([[p]]), torch.tensor([[t]]), torch.tensor([[w]]))
    with pytest.raises(ValueError, match="position 0"):
        build_plan(*one(0, 5), L=20, V=50)
    build_plan(*one(0, 5, 0.0), L=20, V=50)                       # the reference's padding: position 0 with weight 0
    with pytest.raises(ValueError, match="outside the sequence"):
        build_plan(*one(20, 5), L=20, V=50)
    with pytest.raises(ValueError, match="valid length"):
        build_plan(*one(12, 5), L=20, V=50, valid_len=[12])
    build_plan(*one(11, 5), L=20, V=50, valid_len=[12])
    for bad in (-1, 50):
        with pytest.raises(ValueError, match="vocabulary"):
            build_plan(*one(3, bad), L=20, V=50)
    with pytest.raises(ValueError, match="weights"):
        build_plan(*one(3, 5, -1.0), L=20, V=50)
    with pytest.raises(ValueError, match="shape"):
        build_plan(torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 3), L=20, V=50)


# ------------------------------------------------------------------------------------------------ data helper
def test_data_helper_layout_and_counts():
    N, max_len, max_pred = 4, 120, 10
    lens = [1, 3, 4, 10, 100]
    want_n = [1, 1, 1, 2, 10]                                     # min(10, max(1, int(round(len * 0.15)))): round(0.6)=1, round(1.5)=2
    assert [min(max_pred, max(1, int(round(n * 0.15)))) for n in lens] == want_n
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(200, 300, (5, 100), generator=g)
    b = mv.data.seq2seq_finetune_batch(ids, lens, N, max_len, max_pred=max_pred, mask_prob=0.15, mode="s2s", generator=g)
    T = max_len - N - 2
    assert tuple(b["input_txt"].shape) == (5, T) and tuple(b["masked_pos"].shape) == (5, max_pred)
    assert b["attn_mask"].L == max_len and b["attn_mask"].host_desc()[:, 0].tolist() == [1] * 5
    assert b["attn_mask"].host_desc()[:, 2].tolist() == [N + 2 + n + 1 for n in lens]
    for s, (n, k) in enumerate(zip(lens, want_n)):
        w, pos, lab = b["masked_weights"][s], b["masked_pos"][s], b["masked_lm_labels"][s]
        assert w.tolist() == [1.0] * k + [0.0] * (max_pred - k)
        assert pos[k:].tolist() == [0] * (max_pred - k) and lab[k:].tolist() == [0] * (max_pred - k)      # padding layout
        assert int(b["input_txt"][s, n]) in (mv.data.SEP, mv.data.MASK) and b["input_txt"][s, n + 1:].tolist() == [0] * (T - n - 1)
        assert b["segment"][s].tolist() == [1] * (n + 1) + [0] * (T - n - 1)
        for j in range(k):
            t = int(pos[j]) - N - 2
            assert 0 <= t <= n and int(b["input_txt"][s, t]) == mv.data.MASK
            assert int(lab[j]) == (int(ids[s, t]) if t < n else mv.data.SEP)                               # label = the original id
    assert mv.data.seq2seq_finetune_batch(ids, lens, N, max_len, mode="bi", generator=g)["attn_mask"].host_desc()[0, 0] == 4
    assert mv.data.seq2seq_finetune_batch(ids, lens, N, max_len, mode="bar", generator=g)["attn_mask"].host_desc()[0, 0] == 2
    with pytest.raises(ValueError):
        mv.data.seq2seq_finetune_batch(ids, lens, N, max_len, mode="full", generator=g)


def test_data_helper_lists_the_last_sep_half_of_the_time():
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(200, 300, (2000, 20), generator=g)
    b = mv.data.seq2seq_finetune_batch(ids, [20] * 2000, 2, 40, max_pred=3, generator=g)
    last = 2 + 2 + 20
    final = b["masked_pos"][:, 2] == last                          # n_pred = 3: the final slot
    assert abs(float(final.float().mean()) - 0.5) < 0.05
    dup = ((b["masked_pos"][:, :2] == last).any(1) & final)        # ... and then it can be listed twice
    assert int(dup.sum()) > 0


# ------------------------------------------------------------------------------------------------ export and ABI
def test_class_is_exported():
    assert mv.CXRBertForReportFinetune is mv.report_finetune.CXRBertForReportFinetune
    assert "CXRBertForReportFinetune" in mv.__all__


def test_new_symbols_are_declared_exported_and_prototyped():
    src = open(os.path.join(ROOT, "include", "medvill.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/medvill.h"
        assert hasattr(raw, name)
        assert len(_lib.PROTOTYPES[name]) == len([a for a in m.group(1).split(",") if a.strip()])
    assert _lib.load().mv_abi_version() == _lib.ABI_VERSION == 6
    assert re.search(r"#define\s+MV_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "medvill.h")).read())


def _fwd(lib, logits=P, ld=304, U=4, V=300, row_ptr=P, labels=P, n=6, ls=0.1, el=P, hit=P, rs=P):
    return lib.mv_lm_loss_fwd(logits, ld, U, V, row_ptr, labels, n, ls, el, hit, rs, None)


def _sel(lib, el=P, w=P, s=P, hit=P, n=6, B=4, k=3, keep=P, stats=P, inv=P):
    return lib.mv_lm_loss_select(el, w, s, hit, n, B, k, keep, stats, inv, None)


def _bwd(lib, logits=P, ld=304, U=4, V=300, row_ptr=P, labels=P, w=P, s=P, n=6, ls=0.1, rs=P, keep=P, inv=P, g=P, S=None, d=P, dt=0,
         ldd=304):
    return lib.mv_lm_loss_bwd(logits, ld, U, V, row_ptr, labels, w, s, n, ls, rs, keep, inv, g, S, d, dt, ldd, None)


def test_host_side_argument_rejects():
    lib = _lib.load()
    for f in (_fwd, _bwd):
        assert f(lib, logits=None) == E_ARG and f(lib, row_ptr=None) == E_ARG and f(lib, labels=None) == E_ARG
        assert f(lib, ld=299) == E_ARG and f(lib, U=-1) == E_ARG and f(lib, n=-1) == E_ARG and f(lib, V=0) == E_ARG
        assert f(lib, V=2, ld=8, ls=0.1) == E_ARG                  # smoothing spreads over V - 2 columns
        assert f(lib, ls=-0.1) == E_ARG and f(lib, ls=1.5) == E_ARG
        assert f(lib, U=0, n=0, logits=None, row_ptr=None, labels=None) == 0          # nothing to do: no launch
    assert _fwd(lib, el=None) == E_ARG and _fwd(lib, rs=None) == E_ARG
    assert _bwd(lib, w=None) == E_ARG and _bwd(lib, s=None) == E_ARG and _bwd(lib, rs=None) == E_ARG and _bwd(lib, keep=None) == E_ARG
    assert _bwd(lib, inv=None) == E_ARG and _bwd(lib, g=None) == E_ARG and _bwd(lib, d=None) == E_ARG
    assert _bwd(lib, dt=7) == E_DTYPE and _bwd(lib, ldd=296) == E_SHAPE
    assert _sel(lib, keep=None) == E_ARG and _sel(lib, stats=None) == E_ARG and _sel(lib, inv=None) == E_ARG
    assert _sel(lib, el=None) == E_ARG and _sel(lib, w=None) == E_ARG and _sel(lib, s=None) == E_ARG
    assert _sel(lib, B=0) == E_ARG and _sel(lib, k=-1) == E_ARG and _sel(lib, n=-1) == E_ARG and _sel(lib, B=2049) == E_SHAPE


def test_wrappers_refuse_cpu_tensors():
    z = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mv.hip_ops.lm_loss_fwd(z, torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 0.1)


# ------------------------------------------------------------------------------------------------ state dict
def test_state_dict_is_the_finetune_layout_of_cxrbert():
    m = mv.CXRBertForReportFinetune(TINY, dtype=torch.float32, device="cpu", label_smoothing=0.1)
    sd, base = m.state_dict(), m.bert.state_dict()
    assert list(sd) == list(to_finetune_keys(base))
    assert any(k.startswith("cls.predictions.") for k in sd) and not any(k.startswith(("enc.", "mlm.")) for k in sd)
    assert [n for n, _ in m.named_parameters()] == ["bert." + n for n, _ in m.bert.named_parameters()]


def test_save_load_round_trips_and_generation_reads_the_directory(tmp_path):
    torch.manual_seed(3)
    m = mv.CXRBertForReportFinetune(TINY, dtype=torch.float32, device="cpu", label_smoothing=0.1)
    m.save_pretrained(str(tmp_path / "ft"))
    m2 = mv.CXRBertForReportFinetune.from_pretrained(str(tmp_path / "ft"), dtype=torch.float32, device="cpu")
    assert m2.label_smoothing == 0.1                               # config.json carries it, as config.label_smoothing of the reference
    want = m.bert.state_dict()
    for k, v in m2.bert.state_dict().items():
        assert torch.equal(v, want[k]), k
    # a pretraining checkpoint (CXRBERT.save_pretrained: enc.* / mlm.* / itm.*)
    m.bert.save_pretrained(str(tmp_path / "pre"))
    m3 = mv.CXRBertForReportFinetune.from_pretrained(str(tmp_path / "pre"), dtype=torch.float32, device="cpu", label_smoothing=0.2)
    assert m3.label_smoothing == 0.2 and all(torch.equal(v, want[k]) for k, v in m3.bert.state_dict().items())
    r = m3.load_state_dict(m.state_dict())
    assert not r.missing_keys and not r.unexpected_keys
    # the decoder side reads the fine-tuned directory: identical tensors; pretraining-layout loads stay as they are
    for cls in (mv.CXRBertForGeneration, mv.CXRBERT):
        for d in ("ft", "pre"):
            g = cls.from_pretrained(str(tmp_path / d), dtype=torch.float32, device="cpu")
            got = (g.bert if cls is mv.CXRBertForGeneration else g).state_dict()
            assert all(torch.equal(got[k], v) for k, v in want.items()), (cls.__name__, d)


def test_forward_needs_the_three_lists_and_refuses_data_parallel_use(monkeypatch):
    m = mv.CXRBertForReportFinetune(TINY, dtype=torch.float32, device="cpu")
    z = torch.zeros(2, 5, dtype=torch.int64)
    args = (z[:, :1], z, torch.ones(2, 11, 11, dtype=torch.int64), z, (torch.zeros(2, 4, 2048), z[:, :4]), z[:, :1])
    with pytest.raises(ValueError, match="masked_lm_labels"):
        m(*args, masked_pos=z)
    with pytest.raises(ValueError):
        mv.CXRBertForReportFinetune(TINY, device="cpu", label_smoothing=1.5)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    lists = dict(masked_lm_labels=torch.ones(2, 2, dtype=torch.int64), masked_pos=torch.full((2, 2), 7), masked_weights=torch.ones(2, 2))
    with pytest.raises(RuntimeError, match="data-parallel"):
        m(*args, **lists)


# ------------------------------------------------------------------------------------------------ BertAdam's table
def test_bertadam_marks_the_unreached_tensors_inactive():
    m = mv.CXRBertForReportFinetune(TINY, dtype=torch.float32, device="cpu")
    opt = mv.optim.BertAdam(m.parameters(), lr=1e-3, weight_decay=0.01)
    names = m.bert._param_names
    ent = opt._entries()
    assert len(ent) == len(names)
    for n, e in zip(names, ent):
        assert e[3] == (not n.startswith(("itm.", "enc.pooler."))), n
    assert sum(1 for e in ent if not e[3]) == 4 and opt._task is None
    # a bare CXRBERT: every tensor active, as before
    bare = mv.CXRBERT(TINY, dtype=torch.float32, device="cpu")
    assert all(e[3] for e in mv.optim.BertAdam(bare.parameters(), lr=1e-3)._entries())
    # the reference is weak: an encoder that outlives its task module is a bare CXRBERT again
    bert = m.bert
    del m, opt
    import gc
    gc.collect()
    assert all(e[3] for e in mv.optim.BertAdam(bert.parameters(), lr=1e-3)._entries())
