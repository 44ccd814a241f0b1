"""Host half of the grouped weight-gradient launch (include/medvill.h, mv_gemm_grouped_*): the table builder, the tail rule and the
unit -> (problem, tile, K-slice) map, through the C ABI.  mv_gemm_grouped_decode runs the very function the kernel decodes a unit with
(csrc/mv_gemm_group.h is compiled for both sides), so what is checked here is the map the GPU uses.  Pointers are never dereferenced:
every call returns before a launch.  (tests/native/group_plan_check.cpp drives the same header as a stand-alone program for the
host sanitizers.)"""
import ctypes as C

import pytest

import medvill_amd  # noqa: F401
from medvill_amd import _lib
from medvill_amd.hip_ops import GroupProblem

E_ARG, E_SHAPE, E_DTYPE, E_WS = -1, -2, -3, -4
F32, BF16, F16 = 0, 1, 2
P = 0x10000         # a non-null, 16-byte aligned address that is never dereferenced
G = 256


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def problems(shapes, base=P):
    """(No, Ko, rows) -> GroupProblem array with distinct fake pointers, tight leading dimensions rounded to 8."""
    arr = (GroupProblem * len(shapes))()
    for i, (No, Ko, rows) in enumerate(shapes):
        lda, ldb = (No + 7) // 8 * 8, (Ko + 7) // 8 * 8
        arr[i] = GroupProblem(base + 0x100000 * (3 * i), base + 0x100000 * (3 * i + 1), base + 0x100000 * (3 * i + 2), lda, ldb, Ko, No, Ko, rows)
    return arr


def fill(lib, shapes, n_blocks=G, dtype=BF16):
    arr = problems(shapes)
    nb = lib.mv_gemm_grouped_table_bytes(len(shapes))
    assert nb == 64 + 64 * len(shapes)
    buf = C.create_string_buffer(nb)
    assert lib.mv_gemm_grouped_fill(dtype, len(shapes), arr, n_blocks, buf, nb) == 0
    return buf


def header(buf):
    w = (C.c_int * 16).from_buffer(buf)
    return {"count": w[1], "dtype": w[2], "n_blocks": w[3], "units": w[4], "direct": w[5], "tail": w[6], "split": w[7]}


def decode_all(lib, buf):
    h = header(buf)
    out = (C.c_int * 7)()
    res = []
    for u in range(h["direct"] + h["tail"] * h["split"]):
        assert lib.mv_gemm_grouped_decode(buf, u, out) == 0
        res.append(tuple(out))
    assert lib.mv_gemm_grouped_decode(buf, len(res), out) == E_ARG and lib.mv_gemm_grouped_decode(buf, -1, out) == E_ARG
    return h, res


def check_plan(lib, shapes, n_blocks=G):
    """Every tile of every problem is computed exactly once over its whole contraction: unsplit tiles by one unit, tail tiles by `split`
    units whose K ranges tile [0, rows) in multiples of 64."""
    buf = fill(lib, shapes, n_blocks)
    h, units = decode_all(lib, buf)
    tiles = [((No + 255) // 256) * ((Ko + 255) // 256) for No, Ko, _ in shapes]
    U = sum(tiles)
    assert h["units"] == U and h["direct"] + h["tail"] == U and h["count"] == len(shapes) and h["n_blocks"] == n_blocks
    seen = {}
    for (prob, m0, n0, kbeg, kend, sl, tile) in units:
        No, Ko, rows = shapes[prob]
        assert 0 <= m0 < No and 0 <= n0 < Ko and m0 % 256 == 0 and n0 % 256 == 0
        assert sum(tiles[:prob]) <= tile < sum(tiles[:prob + 1])
        seen.setdefault((prob, m0, n0), []).append((sl, kbeg, kend, tile))
    assert len(seen) == U                                   # every (problem, tile origin) shows up ...
    flat = set()
    for (prob, m0, n0), parts in seen.items():
        rows = shapes[prob][2]
        assert len({t for *_, t in parts}) == 1             # ... under one flat tile index
        flat.add(parts[0][3])
        if parts[0][3] < h["direct"]:
            assert parts == [(-1, 0, rows, parts[0][3])]
        else:
            assert sorted(s for s, *_ in parts) == list(range(h["split"]))
            pos = 0
            for s, kbeg, kend, _ in sorted(parts):
                assert kbeg == min(pos, rows) and kbeg <= kend <= rows and (kend == rows or (kend - kbeg) % 64 == 0)
                pos = max(pos, kend)
            assert pos == rows
    assert flat == set(range(U))
    ws = lib.mv_gemm_grouped_workspace_bytes(buf)
    assert ws == (h["tail"] * h["split"] * 256 * 256 * 4 if h["split"] > 1 else 0)
    return h


def layer_set(rows=25483, H=768, I=3072, layers=11):
    return [s for _ in range(layers) for s in ((H, I, rows), (I, H, rows), (H, H, rows), (3 * H, H, rows))]


@pytest.mark.parametrize("U", [1, G - 1, G, G + 1])
def test_unit_counts_around_one_round(lib, U):
    # one problem of U row tiles and one column tile, split over two problems so that a problem boundary falls inside the list
    shapes = [(256 * U, 200, 4100)] if U == 1 else [(256 * (U - 1), 256, 4100), (130, 70, 333)]
    h = check_plan(lib, shapes)
    # U = 1 and G + 1 leave a single unit for the last round: no factor <= 8 fills 70 % of it; G - 1 fills its round; G has no remainder
    assert (h["direct"], h["tail"], h["split"]) == (U, 0, 1)


def test_the_eleven_layer_problem_set(lib):
    shapes = layer_set()
    h = check_plan(lib, shapes)
    # 1,188 tiles: four full rounds of 256, then 164 tiles x 3 slices = 492 units = 96 % of two rounds (x1: 64 %, x2: 64 %)
    assert (h["units"], h["direct"], h["tail"], h["split"]) == (1188, 1024, 164, 3)
    assert lib.mv_gemm_grouped_workspace_bytes(fill(lib, shapes)) == 164 * 3 * 256 * 256 * 4


@pytest.mark.parametrize("R,G_,split", [(100, 256, 2), (180, 256, 1), (164, 256, 3), (1, 3, 3), (2, 5, 2), (3, 4, 1), (0, 7, 1), (40, 256, 5),
                                        (10, 256, 1)])
def test_tail_rule(lib, R, G_, split):
    """R units left after the full rounds are cut by the smallest factor <= 8 that fills the rounds they occupy to >= 70 %; else unsplit."""
    s = next((s for s in range(1, 9) if 10 * R * s >= 7 * -(-R * s // G_) * G_), 1) if R else 1
    assert s == split                                       # the rule as stated, restated
    shapes = [(256 * (G_ + R), 256, 2048)]
    h = check_plan(lib, shapes, G_)
    assert (h["direct"], h["tail"], h["split"]) == ((G_ + R, 0, 1) if split == 1 else (G_, R, split))


def test_short_contraction_in_the_tail_has_empty_slices(lib):
    shapes = [(256 * 7, 256, 640), (128, 64, 100)]          # 8 units on 7 blocks: the last tile is cut 5 ways, 100 rows fill 2 slices of 64
    buf = fill(lib, shapes, 7)
    h, units = decode_all(lib, buf)
    assert (h["direct"], h["tail"], h["split"]) == (7, 1, 5)
    parts = sorted((sl, kbeg, kend) for prob, _, _, kbeg, kend, sl, _ in units if sl >= 0)
    assert parts == [(0, 0, 64), (1, 64, 100), (2, 100, 100), (3, 100, 100), (4, 100, 100)]
    check_plan(lib, shapes, 7)


def test_units_that_run_together_on_one_xcd_are_neighbours(lib):
    """Blocks b, b + 8, ... share an L2 (one XCD); in one round they work on consecutive tiles of the flat list."""
    buf = fill(lib, layer_set())
    _, units = decode_all(lib, buf)
    for rnd in range(4):
        for xcd in range(8):
            tiles = sorted(units[rnd * G + b][6] for b in range(xcd, G, 8))
            assert tiles == list(range(tiles[0], tiles[0] + 32))
            assert len({units[rnd * G + b][0] for b in range(xcd, G, 8)}) <= 3       # 32 tiles span at most the 9-tile product and its two neighbours


def test_fill_rejects(lib):
    nb = lib.mv_gemm_grouped_table_bytes(2)
    buf = C.create_string_buffer(nb)
    ok = [(256, 256, 320), (200, 136, 333)]
    assert lib.mv_gemm_grouped_table_bytes(0) == 0 and lib.mv_gemm_grouped_table_bytes(-3) == 0
    assert lib.mv_gemm_grouped_fill(BF16, 2, None, G, buf, nb) == E_ARG
    assert lib.mv_gemm_grouped_fill(BF16, 2, problems(ok), G, None, nb) == E_ARG
    assert lib.mv_gemm_grouped_fill(BF16, 0, problems(ok), G, buf, nb) == E_ARG
    assert lib.mv_gemm_grouped_fill(BF16, 2, problems(ok), -1, buf, nb) == E_ARG
    assert lib.mv_gemm_grouped_fill(F32, 2, problems(ok), G, buf, nb) == E_DTYPE and lib.mv_gemm_grouped_fill(7, 2, problems(ok), G, buf, nb) == E_DTYPE
    assert lib.mv_gemm_grouped_fill(BF16, 2, problems(ok), G, buf, nb - 1) == E_WS
    assert lib.mv_gemm_grouped_fill(BF16, 257, problems([(64, 64, 64)] * 257), G, buf, nb) == E_SHAPE
    for field, value, rc in (("A", None, E_ARG), ("B", None, E_ARG), ("C", None, E_ARG), ("No", 0, E_ARG), ("rows", -1, E_ARG),
                             ("A", P + 8, E_SHAPE), ("B", P + 2, E_SHAPE), ("C", P + 2, E_SHAPE), ("lda", 204, E_SHAPE), ("lda", 128, E_SHAPE),
                             ("ldb", 100, E_SHAPE), ("ldc", 100, E_SHAPE)):
        arr = problems(ok)
        setattr(arr[1], field, value)
        assert lib.mv_gemm_grouped_fill(BF16, 2, arr, G, buf, nb) == rc, (field, value)
    # an operand of 2 GiB or more cannot be addressed through a buffer resource: sizes only, nothing is allocated
    big = problems([(768, 768, 1 << 21)])                   # (2^21 - 1) * 768 * 2 bytes > 2 GiB
    assert lib.mv_gemm_grouped_fill(BF16, 1, big, G, buf, nb) == E_SHAPE
    assert lib.mv_gemm_grouped_fill(BF16, 1, problems([(768, 768, 1 << 20)]), G, buf, nb) == 0


def test_launch_rejects_before_it_touches_the_device(lib):
    shapes = [(256, 256, 320), (512, 256, 448), (768, 256, 448), (200, 136, 333)]
    buf = fill(lib, shapes, 3)                               # 7 units on 3 blocks: one tail tile cut 3 ways -> a workspace is needed
    need = lib.mv_gemm_grouped_workspace_bytes(buf)
    assert need == 3 * 256 * 256 * 4
    call = lambda dtype=BF16, count=4, th=buf, td=P, ws=P, wsb=need: lib.mv_gemm_grouped_tn(dtype, count, th, td, ws, wsb, 0, None, None)  # noqa: E731
    assert call(th=None) == E_ARG and call(td=None) == E_ARG                 # a null table
    assert call(count=0) == E_ARG and call(count=3) == E_ARG                 # a zero count; a count that is not the table's
    assert call(dtype=F32) == E_DTYPE and call(dtype=9) == E_DTYPE           # a bad dtype
    assert call(dtype=F16) == E_DTYPE                                         # the table was planned for bf16 operands
    assert call(td=P + 4) == E_SHAPE
    assert call(ws=None) == E_WS and call(wsb=need - 1) == E_WS
    assert call(th=C.create_string_buffer(len(buf))) == E_ARG                # not a table
    assert lib.mv_gemm_grouped_workspace_bytes(None) == 0
    # a table that was edited after mv_gemm_grouped_fill is validated again: a misaligned pointer, an operand over 2 GiB
    for word, value, rc in ((16 + 0, P + 8, E_SHAPE), (16 + 11, 1 << 22, E_SHAPE), (16 + 14, 5, E_ARG)):
        bad = C.create_string_buffer(buf.raw, len(buf))
        (C.c_int * (len(buf) // 4)).from_buffer(bad)[word] = value
        assert call(th=bad) == rc, word
