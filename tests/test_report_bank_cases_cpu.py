"""The report bank without a GPU: the numpy restatements of tests/report_bank_cases.py against report_finetune.build_plan and against the
rule's own properties, the distribution of the hash draws, the planted defects the case set must catch, data.ReportBank's host side
and the CPU-reachable half of csrc/mv_report.hip's C ABI (every entry validates its arguments before it touches the HIP runtime)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import medvill_amd as mv                                   # noqa: E402
from medvill_amd import _build, _lib                       # noqa: E402
from medvill_amd.report_finetune import build_plan         # noqa: E402
import report_bank_cases as C                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mv_report_draws", "mv_report_assemble", "mv_report_plan")


# ------------------------------------------------------------------------------------------------ plan
def _same_as_build_plan(pos, lab, w, L, V, vl=None):
    got = C.plan(pos, lab, w, L, V, vl)
    ref = build_plan(torch.from_numpy(pos), torch.from_numpy(lab), torch.from_numpy(w), L=L, V=V,
                     valid_len=None if vl is None else torch.from_numpy(vl))
    assert got["counts"].tolist() == [ref["U"], ref["n"], 0, 0]
    for k in ("rows", "row_ptr", "labels", "sample"):
        assert got[k].dtype == np.int32 and got[k].tolist() == ref[k].tolist(), k
    assert got["weights"].tobytes() == ref["weights"].numpy().tobytes()
    return got


@pytest.mark.parametrize("kind", ["plain", "duplicates", "zero_weight", "label0", "fractional", "all_zero", "valid_len"])
def test_restated_plan_equals_build_plan(kind):
    pos, lab, w, vl = C.plan_case(kind)
    got = _same_as_build_plan(pos, lab, w, 40, 300, vl)
    if kind == "all_zero":
        assert got["counts"].tolist() == [0, 0, 0, 0] and got["row_ptr"].tolist() == [0]
    if kind == "duplicates":
        u = got["rows"].tolist().index(7)                                  # sample 0, position 7: three entries in slot order
        assert got["labels"][got["row_ptr"][u]:got["row_ptr"][u + 1]].tolist() == [11, 11, 12]
        assert got["counts"][1] - got["counts"][0] == 3                    # 3 + 2 entries on 2 rows


@pytest.mark.parametrize("B,P", [(1, 6), (5, 1), (3, 64), (1, 1)])
def test_restated_plan_equals_build_plan_at_the_edge_shapes(B, P):
    for kind in ("plain", "zero_weight", "fractional") + (("duplicates",) if P >= 3 else ()):
        pos, lab, w, vl = C.plan_case(kind, B=B, P=P, seed=B + P)
        _same_as_build_plan(pos, lab, w, 40, 300, vl)


@pytest.mark.parametrize("kind", C.BAD_KINDS)
def test_bad_entries_are_counted_and_dropped(kind):
    L, V = 40, 300
    pos, lab, w, vl = C.plan_case("duplicates")
    vl = C.spoil(kind, pos, lab, w, vl, L, V)
    got = C.plan(pos, lab, w, L, V, vl)
    with pytest.raises(ValueError):                                        # the host plan refuses the same list
        build_plan(torch.from_numpy(pos), torch.from_numpy(lab), torch.from_numpy(w), L=L, V=V,
                   valid_len=None if vl is None else torch.from_numpy(vl))
    w[1, 2] = 0.0                                                          # without the entry: the same plan
    want = C.plan(pos, lab, w, L, V, vl)
    assert got["counts"].tolist() == [want["counts"][0], want["counts"][1], 1, 0]
    for k in ("rows", "row_ptr", "labels", "weights", "sample"):
        assert got[k].tolist() == want[k].tolist(), k


# ------------------------------------------------------------------------------------------------ assemble
def test_n_pred_table_rounds_like_python():
    # text tokens (without the [SEP]) -> predictions at mask_prob 0.15: 10 -> round(1.5) = 2, 30 -> round(4.5) = 4, 3 -> round(0.45) = 0 -> 1
    table = {3: 1, 10: 2, 30: 4, 1: 1, 17: 3, 50: 8, 67: 10, 200: 10, 252: 10}
    for toks, want in table.items():
        assert C.n_pred_of(toks + 1) == want, toks
    assert C.n_pred_of(31, max_pred=3) == 3 and C.n_pred_of(1) == 1
    bank = mv.data.ReportBank(device="cpu", max_pred=10, mask_prob=0.15)
    T = 254
    lens = torch.tensor([t + 1 for t in table])
    ids = torch.zeros((len(table), T), dtype=torch.int64)
    bank.add_reports(ids[:4], lens[:4]).add_reports(ids[4:], lens[4:])         # in two parts: the table is per item
    assert bank.n_pred.dtype == torch.int32 and bank.n_pred.tolist() == list(table.values())
    assert bank._len_host.tolist() == lens.tolist() and bank.n_texts == len(table)


def _assemble_cases():
    """(bank, idx, max_pred, words): small banks under every kind of draw; idx repeats items and names len = 1 and len = T."""
    out = []
    for T, max_pred, seed in ((2, 1, 0), (3, 3, 1), (17, 10, 2), (17, 64, 3), (65, 10, 4)):
        bank = C.make_bank(6, T, 2, 4, seed, max_pred=max_pred, mask_prob=0.4)
        idx = [0, 1, 2, 3, 1, 5, 4, 0]
        for kind in ("random", "equal", "descending"):
            out.append((bank, idx, max_pred, C.injected_draws(len(idx), T, seed, kind)))
        out.append((bank, idx, max_pred, C.draws(7, seed, len(idx), T)))
    return out


def test_assemble_rule_properties():
    coins = set()
    for bank, idx, max_pred, words in _assemble_cases():
        got = C.assemble(bank, idx, max_pred, words)
        ids, T = bank["txt_ids"], bank["txt_ids"].shape[1]
        N = bank["img_pos"].shape[1]
        for i, d in enumerate(idx):
            ln = int(bank["txt_len"][d])
            p = min(int(bank["n_pred"][d]), max_pred, ln)
            coin = int(words[i, T]) >> 31
            coins.add(coin)
            mp, ml, mw = got["masked_pos"][i], got["masked_lm_labels"][i], got["masked_weights"][i]
            assert mw.tolist() == [1.0] * p + [0.0] * (max_pred - p)
            assert mp[p:].tolist() == [0] * (max_pred - p) and ml[p:].tolist() == [0] * (max_pred - p)      # padded with (0, 0, 0)
            t = mp[:p] - (N + 2)
            assert ((t >= 0) & (t < ln)).all()
            assert ml[:p].tolist() == ids[d, t].tolist()                           # labels: the original ids
            listed = np.zeros(T, bool)
            listed[t] = True
            assert (got["input_txt"][i][listed] == C.MASK).all()                   # 103 at the listed indices and nowhere else
            assert (got["input_txt"][i][~listed] == ids[d][~listed]).all() and not (ids[d] == C.MASK).any()
            assert got["segment"][i].tolist() == [1] * ln + [0] * (T - ln)
            assert got["desc"][i].tolist() == [C.FAMILY_S2S, N + 2, N + 2 + ln]
            if coin and p > 0:
                assert t[p - 1] == ln - 1 and ml[p - 1] == C.SEP                   # the [SEP] takes the last slot
                assert len(set(t[:p - 1].tolist())) == p - 1
            else:
                assert len(set(t.tolist())) == p
            if ln == 1:
                assert t.tolist() == [0] * p and p == 1 and ml[0] == C.SEP         # only the [SEP]
            assert (got["feats"][i] == bank["img_feats"][d]).all() and (got["pos"][i] == bank["img_pos"][d]).all()
    assert coins == {0, 1}


def test_tie_rule_on_injected_draws():
    T, max_pred = 17, 5
    bank = C.make_bank(4, T, 1, 4, 9, max_pred=max_pred, lengths=[T, 9, 1, 12])
    bank["n_pred"][:] = max_pred
    idx = [0, 1, 2, 3]
    for kind, first in (("equal", lambda ln: list(range(ln))), ("descending", lambda ln: list(range(ln))[::-1])):
        words = C.injected_draws(4, T, 0, kind)
        got = C.assemble(bank, idx, max_pred, words)
        for i, d in enumerate(idx):
            ln = int(bank["txt_len"][d])
            p = min(max_pred, ln)
            order = first(ln)
            want = order[:p - 1] + [ln - 1] if i % 2 == 0 else order[:p]          # injected coins: set for even samples
            assert (got["masked_pos"][i][:p] - 3).tolist() == want, (kind, i)
    # len = T with the coin set and every key equal: the [SEP] is listed once, as the last slot, after indices 0 .. p-2
    assert (C.assemble(bank, [0], max_pred, C.injected_draws(1, T, 0, "equal"))["masked_pos"][0] - 3).tolist() == [0, 1, 2, 3, T - 1]


def test_families_and_clamped_indices():
    bank = C.make_bank(3, 5, 2, 4, 1)
    words = C.injected_draws(4, 5, 1)
    got = C.assemble(bank, [-4, 7, 1, 2], 10, words, family=[C.FAMILY_1D, C.FAMILY_BAR, C.FAMILY_S2S, C.FAMILY_1D])
    assert got["desc"][:, 0].tolist() == [4, 2, 1, 4]
    ref = C.assemble(bank, [0, 2, 1, 2], 10, words)
    for k in ("input_txt", "masked_pos", "feats"):
        assert (got[k] == ref[k]).all()


# ------------------------------------------------------------------------------------------------ distribution of the hash draws
def _selection(words, ln, p):
    """Vectorised chosen_indices for samples of one length: -> (chosen [n, p], coin [n])."""
    order = np.argsort(words[:, :ln], axis=1, kind="stable")               # (word, index): ties to the lower index
    coin = (words[:, -1] >> np.uint64(31)).astype(bool)
    chosen = order[:, :p].copy()
    chosen[coin, p - 1] = ln - 1
    return chosen, coin


@pytest.mark.parametrize("ln,p", [(8, 3), (31, 5), (200, 10)])
def test_hash_draws_select_every_index_at_the_rules_rate(ln, p):
    steps, slots = 8, 4096
    n = steps * slots
    hits = np.zeros(ln, np.int64)
    coins = dups = 0
    for step in range(steps):
        words = C.draws(0x5EED, step, slots, ln)                              # T = len: every index is a candidate
        chosen, coin = _selection(words, ln, p)
        if step == 0:
            for i in range(16):                                            # the vectorised form is the restatement
                assert chosen[i].tolist() == C.chosen_indices(words[i], ln, p, ln)
        sel = np.zeros((slots, ln), bool)
        np.put_along_axis(sel, chosen, True, axis=1)
        hits += sel.sum(0)
        coins += int(coin.sum())
        dups += int((coin & (chosen[:, :p - 1] == ln - 1).any(1)).sum())

    def sigmas(count, q):
        return abs(count / n - q) / np.sqrt(q * (1 - q) / n)

    q = (p - 0.5) / ln
    worst = max(sigmas(hits[t], q) for t in range(ln - 1))
    print(f"len {ln} p {p}: worst index {worst:.2f} sd, coin {sigmas(coins, 0.5):.2f} sd, duplicate {sigmas(dups, (p - 1) / (2 * ln)):.2f} sd")
    assert worst < 5.0
    assert sigmas(coins, 0.5) < 5.0
    assert sigmas(dups, (p - 1) / (2.0 * ln)) < 5.0


def test_draws_depend_on_key_and_step_and_fill_32_bits():
    a, b, c = C.draws(1, 0, 4, 9), C.draws(1, 1, 4, 9), C.draws(2, 0, 4, 9)
    assert a.shape == (4, 10) and (a != b).any() and (a != c).any() and (a == C.draws(1, 0, 4, 9)).all()
    assert int(a.max()) < 1 << 32 and int(C.draws(3, 5, 64, 63).max()) > 1 << 31
    assert C.derive_keys(0, 0) == (0, 0) and C.derive_keys(5, 1) == ((5 ^ 0x7F4A7C15) & 0xFFFFFFFF, 0x9E3779B9)


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("defect", ["tie_high", "coin_inverted", "no_sep"])
def test_case_set_catches_a_planted_assemble_defect(defect):
    caught = 0
    for bank, idx, max_pred, words in _assemble_cases():
        good, bad = C.assemble(bank, idx, max_pred, words), C.assemble(bank, idx, max_pred, words, defect=defect)
        caught += int(any((good[k] != bad[k]).any() for k in ("masked_pos", "masked_lm_labels", "input_txt")))
    assert caught >= 2, defect


@pytest.mark.parametrize("defect", ["drop_duplicate", "slot_order"])
def test_case_set_catches_a_planted_plan_defect(defect):
    pos, lab, w, vl = C.plan_case("duplicates")
    good, bad = C.plan(pos, lab, w, 40, 300), C.plan(pos, lab, w, 40, 300, defect=defect)
    assert good["labels"].tolist() != bad["labels"].tolist()


# ------------------------------------------------------------------------------------------------ ABI
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "medvill.h")).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(mv_report_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_new_symbols_are_declared_exported_and_prototyped():
    decl = _declared()
    assert set(decl) == set(NEW)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and len(_lib.PROTOTYPES[name]) == decl[name], name
    assert "mv_report.hip" in _build.SOURCES
    from medvill_amd import hip_ops as ops
    assert all(callable(getattr(ops, f)) for f in ("report_draws", "report_assemble", "report_plan"))
    assert callable(mv.CXRBertForReportFinetune.fit_step) and callable(mv.CXRBertForReportFinetune.eval_step)


E_ARG, E_SHAPE, E_DTYPE = -1, -2, -3
PTR = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced: every call below must return before a launch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_report_draws_rejects(lib):
    dr = lambda **k: lib.mv_report_draws(1, 2, k.get("B", 4), k.get("T", 9), k.get("out", PTR), None)
    assert dr(out=None) == E_ARG and dr(B=0) == E_ARG and dr(B=-1) == E_ARG and dr(T=0) == E_ARG and dr(T=-2) == E_ARG
    assert dr(T=1025) == E_SHAPE and dr(B=1 << 21, T=1024) == E_SHAPE                       # LDS words; 32-bit hash counters


def test_report_assemble_rejects(lib):
    def asm(**k):
        g = lambda name, default=PTR: k.get(name, default)
        return lib.mv_report_assemble(g("ids"), g("len"), g("n_pred"), g("n", 5), g("img"), g("dt", 2), g("ipos"), g("idx"),
                                      g("family", None), g("B", 3), g("N", 3), g("T", 6), g("F", 8), g("max_pred", 4), 1, 2,
                                      g("draws", None), g("txt"), g("seg"), g("desc"), g("feats"), g("pos"), g("mpos"), g("mlab"),
                                      g("mw"), None)
    for name in ("ids", "len", "n_pred", "img", "ipos", "idx", "txt", "seg", "desc", "feats", "pos", "mpos", "mlab", "mw"):
        assert asm(**{name: None}) == E_ARG, name
    for name in ("n", "B", "N", "T", "F", "max_pred"):
        assert asm(**{name: 0}) == E_ARG and asm(**{name: -2}) == E_ARG, name
    assert asm(dt=3) == E_DTYPE and asm(dt=-1) == E_DTYPE
    assert asm(T=1025) == E_SHAPE and asm(max_pred=65) == E_SHAPE
    assert asm(N=1 << 16, F=1 << 16) == E_SHAPE and asm(B=1 << 21, T=1024) == E_SHAPE


def test_report_plan_rejects(lib):
    def pl(**k):
        g = lambda name, default=PTR: k.get(name, default)
        return lib.mv_report_plan(g("pos"), g("lab"), g("w"), g("vl", None), g("B", 4), g("P", 6), g("L", 64), g("V", 300), g("work"),
                                  g("rows"), g("row_ptr"), g("olab"), g("ow"), g("osample"), g("counts"), None)
    for name in ("pos", "lab", "w", "work", "rows", "row_ptr", "olab", "ow", "osample", "counts"):
        assert pl(**{name: None}) == E_ARG, name
    for name in ("B", "P", "L", "V"):
        assert pl(**{name: 0}) == E_ARG and pl(**{name: -1}) == E_ARG, name
    assert pl(P=65) == E_SHAPE and pl(B=2049) == E_SHAPE and pl(B=2048, L=1 << 21) == E_SHAPE


# ------------------------------------------------------------------------------------------------ ReportBank, host side
def test_report_bank_refusals_on_the_host():
    bank = mv.data.ReportBank(device="cpu", max_pred=4)
    with pytest.raises(ValueError, match="empty"):
        bank.assemble([0])
    ids = torch.zeros((3, 6), dtype=torch.int64)
    bank.add_reports(ids, [2, 6, 1])
    with pytest.raises(ValueError, match="empty"):
        bank.assemble([0])
    bank.add_images((torch.zeros(2, 3, 8), torch.zeros(2, 3, dtype=torch.int64)))
    with pytest.raises(ValueError, match="3 reports"):
        bank.assemble([0])
    bank.add_images((torch.zeros(1, 3, 8), torch.zeros(1, 3, dtype=torch.int64)))
    with pytest.raises(IndexError):
        bank.assemble([0, 3])
    with pytest.raises(IndexError):
        bank.assemble([-1])
    with pytest.raises(ValueError, match="mode"):
        bank.assemble([0, 1], mode="full")
    with pytest.raises(ValueError, match="mode"):
        bank.assemble([0, 1], mode=["s2s"])
    with pytest.raises(ValueError):
        bank.add_reports(ids, [2, 7, 1])                                    # a length past the row
    with pytest.raises(ValueError):
        mv.data.ReportBank(device="cpu", max_pred=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # a missing kernel is an error, not a host loop
        bank.assemble([0, 1])
