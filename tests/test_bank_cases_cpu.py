"""The feature gather the three bank kernels share (csrc/mv_bank.h), without a GPU: the launcher's chunk plan, restated in
tests/bank_cases.py over the header's constants, applied to every (N, F, element size, alignment) the pair-assembly test
(test_retrieval_gpu.py) and the report sweep (test_report_bank_sweep_gpu.py) run.  Each list reaches every branch of the plan and of the
copy loop but the capped grid; that one needs a row beyond 64 MiB, which the VQA sweep holds once for all three kernels
(test_vqa_bank_cases_cpu.py).  A condition on the inputs, not a measurement."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bank_cases as BC                 # noqa: E402
import report_bank_cases as RB          # noqa: E402
import retrieval_cases as RC            # noqa: E402

K = BC.source_constants()


def _pair_cases():
    """The bank itself (a fresh allocation: aligned) and the view the test cuts PAIR_VIEW_OFFSET elements into it."""
    for N, S, F in RC.PAIR_SHAPES:
        for dtn in RC.PAIR_DTYPES:
            item = BC.ITEMSIZE[dtn]
            yield N, F, item, True
            yield N, F, item, (RC.PAIR_VIEW_OFFSET * item) % K["VEC_BYTES"] == 0


def _report_cases():
    """Every output of a sweep case starts `guard` elements into its buffer."""
    for T, B, max_pred, N, F, dtn, kind in RB.SWEEP + RB.COPY_CASES:
        item = BC.ITEMSIZE[dtn]
        guard = RB.GUARD_ODD if kind == "odd-guard" else RB.GUARD
        yield N, F, item, (guard * item) % K["VEC_BYTES"] == 0


def test_the_header_holds_the_plans_constants():
    assert {"NT", "VEC_BYTES", "UNROLL", "CHUNK_BYTES", "MAX_CHUNKS"} <= set(K)
    assert K["CHUNK_BYTES"] % (K["VEC_BYTES"] * K["UNROLL"] * K["NT"]) == 0        # a full chunk is whole unrolled rounds


@pytest.mark.parametrize("cases", [_pair_cases, _report_cases], ids=["pair", "report"])
def test_the_case_list_reaches_every_branch_but_the_capped_grid(cases):
    seen = set()
    for N, F, item, aligned in cases():
        plan = BC.launch_plan(N, F, item, aligned, K)
        assert plan["chunks"] <= K["MAX_CHUNKS"] and plan["chunk"] * plan["chunks"] >= N * F > plan["chunk"] * (plan["chunks"] - 1)
        if plan["vec"]:
            assert plan["chunk"] % (K["VEC_BYTES"] // item) == 0
        seen |= plan["branches"]
    assert seen == BC.ALL_BRANCHES - {"large_chunks"}, (BC.ALL_BRANCHES - seen, seen - BC.ALL_BRANCHES)


def test_the_added_shapes_end_in_the_tails_they_are_named_for():
    per_round = K["UNROLL"] * K["NT"]
    for N, F, item, last in ((5, 4100, 4, per_round + 5), (9, 4104, 2, 521)):       # vectors of the last chunk
        plan = BC.launch_plan(N, F, item, True, K)
        assert plan["chunks"] > 1 and (N * F - plan["chunk"] * (plan["chunks"] - 1)) * item // K["VEC_BYTES"] == last
        assert any((N, F) == (n, f) and BC.ITEMSIZE[dtn] == item for (n, s, f) in RC.PAIR_SHAPES for dtn in RC.PAIR_DTYPES)
        assert any((N, F, BC.ITEMSIZE[c[5]]) == (c[3], c[4], item) for c in RB.COPY_CASES)
