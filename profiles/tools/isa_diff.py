"""Did a change leave the device code alone?  Compiles every translation unit of this tree and of a git revision to gfx950 assembly
(_build.FLAGS --cuda-device-only -S), cuts the assembly into kernels and compares, per kernel symbol over the whole library, a hash of the
normalised instruction stream and the .amdhsa_* kernel descriptor (registers, LDS, private segment).  Text is compared, nothing is interpreted.
usage: python profiles/tools/isa_diff.py <git-rev> [--json out] [--only SUBSTRING]
       python profiles/tools/isa_diff.py <git-rev> --pair "NEW_UNIT [flags]" "OLD_UNIT [flags]"     (one unit of each tree, the new unit's kernels)
Prints the kernels changed, added and removed; the exit status is non-zero if there is any."""
import argparse
import glob
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = "multi-modality-self-supervision_amd"
_spec = importlib.util.spec_from_file_location("_mv_build", os.path.join(ROOT, PKG, "_build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)

DESC_KEYS = {"vgpr": "next_free_vgpr", "sgpr": "next_free_sgpr", "accum_offset": "accum_offset", "lds": "group_segment_fixed_size",
             "private": "private_segment_fixed_size"}


def compile_unit(job):
    src, extra, out = job
    cmd = [_build._hipcc()] + _build.FLAGS + extra + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-4000:]}")
    return out


def normalise(lines):
    """comments, debug and unwind directives dropped; local labels renamed in order of appearance"""
    names = {}
    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if not line or re.match(r"\.(loc|file|cfi_\w+)\b", line):
            continue
        out.append(re.sub(r"\.L[\w$.]+", lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line))
    return out


def kernels_of(path):
    """{symbol: {"isa": hash, "desc": hash, "vgpr": ..}} of one assembly file"""
    lines = open(path).read().splitlines()
    label = {l.split(":", 1)[0]: n for n, l in enumerate(lines) if re.match(r"[A-Za-z_]\w*:", l)}
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        sym = m.group(1)
        j = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
        end = next(k for k in range(j, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
        d = normalise(lines[i + 1:j])
        body = normalise(lines[label[sym] + 1:i] + lines[j + 1:end])      # (the descriptor is written in front of .Lfunc_end)
        e = {"isa": hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], "desc": hashlib.sha256("\n".join(d).encode()).hexdigest()[:16],
             "instructions": sum(1 for l in body if not l.endswith(":") and not l.startswith("."))}
        for k, name in DESC_KEYS.items():
            v = [l.split()[1] for l in d if l.startswith(".amdhsa_" + name + " ")]
            e[k] = int(v[0]) if v else None
        out[sym] = e
    return out


def library(tree, units, tmp, tag):
    """{symbol: entry} over the units [(file name, extra flags)] of a tree, compiled at most 16 at a time"""
    jobs = [(os.path.join(tree, PKG, "csrc", u), extra, os.path.join(tmp, f"{tag}_{n}.s")) for n, (u, extra) in enumerate(units)]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        outs = list(ex.map(compile_unit, jobs))
    lib = {}
    for (u, _), s in zip(units, outs):
        for sym, e in kernels_of(s).items():
            e["unit"] = u
            if sym in lib and (lib[sym]["isa"], lib[sym]["desc"]) != (e["isa"], e["desc"]):
                raise RuntimeError(f"{sym} differs between {lib[sym]['unit']} and {u} of one tree")
            lib[sym] = e
    return lib


def units_of(tree, only):
    return [(os.path.basename(p), []) for p in sorted(glob.glob(os.path.join(tree, PKG, "csrc", "*.hip"))) if only in os.path.basename(p)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev")
    ap.add_argument("--json")
    ap.add_argument("--only", default="", help="units whose file name contains this")
    ap.add_argument("--pair", nargs=2, metavar=("NEW", "OLD"), help='one unit of each tree with its flags, e.g. "mv_attn_mfma.hip -DATT_PROF=1"')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        os.makedirs(old_tree)
        ar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, PKG + "/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old_tree], input=ar, check=True)
        if a.pair:
            (nu, *nf), (ou, *of) = a.pair[0].split(), a.pair[1].split()
            new, old = library(ROOT, [(nu, nf)], tmp, "new"), library(old_tree, [(ou, of)], tmp, "old")
            old = {s: e for s, e in old.items() if s in new}
        else:
            new, old = library(ROOT, units_of(ROOT, a.only), tmp, "new"), library(old_tree, units_of(old_tree, a.only), tmp, "old")
    same = lambda x, y: all(x[k] == y[k] for k in x if k != "unit")
    changed = sorted(s for s in new if s in old and not same(new[s], old[s]))
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    moved = sum(1 for s in new if s in old and new[s]["unit"] != old[s]["unit"])
    print(f"{len(new)} kernels here, {len(old)} at {a.rev}: {len(changed)} changed, {len(added)} added, {len(removed)} removed; "
          f"{moved} identical in another unit")
    for s in changed:
        n, o = new[s], old[s]
        what = ", ".join(f"{k} {o[k]} -> {n[k]}" for k in n if k != "unit" and n[k] != o[k])
        print(f"  changed  {s} ({o['unit']} -> {n['unit']}): {what}")
    for s in added:
        print(f"  added    {s} ({new[s]['unit']})")
    for s in removed:
        print(f"  removed  {s} ({old[s]['unit']})")
    if a.json:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", a.rev], capture_output=True, text=True, check=True).stdout.strip()
        doc = {"against": rev, "flags": _build.FLAGS + ["--cuda-device-only", "-S"], "pair": a.pair, "changed": changed, "added": added,
               "removed": removed, "kernels": {s: new[s] for s in sorted(new)}}
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 1 if changed or added or removed else 0


if __name__ == "__main__":
    sys.exit(main())
