"""Where the waves of the attention kernels spend their cycles: runs profiles/tools/dominant.py's attention case on a variant library whose
MFMA attention unit is built with -DATT_PROF=1 (csrc/mv_attn.h) and prints the per-phase shader-clock totals of thread 0 of every block.
usage: python profiles/tools/attn_phase.py build      (no GPU needed) compiles csrc/mv_attn_mfma.hip with -DATT_PROF=1 into build/variants/ and
                                                      links it with the other product objects: build/variants/libmedvill_attn_prof.so
       python profiles/tools/attn_phase.py            (on the GPU) runs with that library, or with the one MV_LIB_PATH names"""
import ctypes
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "multi-modality-self-supervision_amd")
VARIANT = os.path.join(PKG, "build", "variants", "libmedvill_attn_prof.so")
UNIT = "mv_attn_mfma.hip"


def build():
    spec = importlib.util.spec_from_file_location("_mv_build", os.path.join(PKG, "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()                                           # the product objects (nothing to do when they are current)
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    obj = os.path.join(os.path.dirname(VARIANT), "mv_attn_mfma_prof.o")
    subprocess.run([b._hipcc()] + b.FLAGS + ["-DATT_PROF=1", "-c", os.path.join(b.CSRC, UNIT), "-o", obj], check=True)
    objs = [obj if s == UNIT else os.path.join(b.OBJ, s.replace(".hip", ".o")) for s in b.SOURCES]
    subprocess.run([b._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", VARIANT] + objs, check=True)
    print(VARIANT)


def run():
    os.environ.setdefault("MV_LIB_PATH", VARIANT)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    from medvill_amd import _lib
    from dominant import make_case

    fn, meta = make_case("attn")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    buf = (ctypes.c_ulonglong * 48)()
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    assert lib.mv_debug_attn_prof(buf) == 0
    reps = 5
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    assert lib.mv_debug_attn_prof(buf) == 0
    names = ["prologue", "wait for the tile's LDS-DMA", "barrier", "tile body", "issue next tile + bookkeeping", "epilogue"]
    for k, kn in enumerate(("forward", "backward dQ", "backward dK/dV")):
        v = [buf[8 * k + i] for i in range(8)]
        nb = max(v[7], 1)
        tot = sum(v[:6])
        print(f"{kn}: {nb // reps} blocks with work per launch, {tot / nb:.0f} shader cycles per block (thread 0)")
        for i in range(6):
            print(f"    {names[i]:32s} {v[i] / nb:9.0f} cycles per block  {100.0 * v[i] / tot:5.1f} %")
    tn = ["score MFMAs (K fragment reads + 8 MFMAs)", "row maximum + cross-half shuffle", "exponentials + row sums", "dropout selects (scalar mask loads)", "P.V (16 transposed reads + 8 MFMAs)"]
    v = [buf[24 + i] for i in range(6)]
    nb = max(buf[7], 1)
    print("forward, inside the tile body (cycles per block, thread 0):")
    for i in range(5):
        print(f"    {tn[i]:44s} {v[i] / nb:9.0f}  {100.0 * v[i] / max(sum(v[:5]), 1):5.1f} %")


if __name__ == "__main__":
    build() if sys.argv[1:] == ["build"] else run()
