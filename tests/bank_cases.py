"""Shared definitions of the bank tests (no GPU, no package import): the chunk plan of csrc/mv_bank.h -- the one launcher plan of
mv_pair_assemble, mv_report_assemble and mv_vqa_assemble -- restated over the header's constants, which are read out of the source file
and not repeated here, and the branches of the plan and of the copy loop a (row, element size, alignment) takes."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-modality-self-supervision_amd", "csrc")
BANK_HEADER = os.path.join(CSRC, "mv_bank.h")
ITEMSIZE = {"f32": 4, "bf16": 2, "f16": 2}


def source_constants(*paths):
    """The `constexpr int NAME = value;` lines of the given files (default: csrc/mv_bank.h)."""
    text = "".join(open(p).read() for p in (paths or (BANK_HEADER,)))
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", text)}


def launch_plan(N, F, itemsize, aligned, k=None):
    """mv_bank.h's chunk_plan, restated over the file's constants: -> dict(chunk, chunks, vec, branches) with `branches` the set of
    paths the launch takes: 'elements' / 'vec' (the copy loop), 'vec_body' / 'vec_tail' / 'ragged_tail' (the unrolled rounds, the
    remainder loop, a remainder that is no multiple of the block), 'one_chunk' / 'many_chunks', 'full_last_chunk' /
    'partial_last_chunk', 'large_chunks' (the grid's second dimension capped), 'misaligned' (whole vectors, bases off 16 bytes)."""
    k = k or source_constants()
    per_vec = k["VEC_BYTES"] // itemsize
    row = N * F
    chunk = k["CHUNK_BYTES"] // itemsize
    chunks = -(-row // chunk)
    br = set()
    if chunks > k["MAX_CHUNKS"]:
        chunk = -(-(-(-row // k["MAX_CHUNKS"])) // per_vec) * per_vec
        chunks = -(-row // chunk)
        br.add("large_chunks")
    vec = row % per_vec == 0 and aligned
    if row % per_vec == 0 and not aligned:
        br.add("misaligned")
    br.add("vec" if vec else "elements")
    br.add("one_chunk" if chunks == 1 else "many_chunks")
    br.add("full_last_chunk" if row % chunk == 0 else "partial_last_chunk")
    if vec:
        round_ = k["UNROLL"] * k["NT"]
        for c in range(chunks):
            n4 = min(row - c * chunk, chunk) // per_vec
            body = n4 // round_ * round_
            if body:
                br.add("vec_body")
            if n4 > body:
                br.add("vec_tail")
                if (n4 - body) % k["NT"]:
                    br.add("ragged_tail")
    return dict(chunk=chunk, chunks=chunks, vec=vec, branches=br)


ALL_BRANCHES = {"elements", "vec", "vec_body", "vec_tail", "ragged_tail", "one_chunk", "many_chunks", "full_last_chunk",
                "partial_last_chunk", "large_chunks", "misaligned"}
