"""mv_attn_probs for one encoder layer at the benchmark shape (A = 12, dh = 64, L = 512; B = 8 and 64): f32 and 16-bit output, per head
and head mean, full mask -- HIP-event timings with the scheme of profiles/tools/dominant.py::time_case (50 warm-up launches, 200 timed
in batches of 10, median batch mean).  Reported per case: microseconds per layer, the achieved rate against the byte model
    B*A*L*L*sizeof(out) written (B*L*L*sizeof(out) with head mean)  +  B*L*3H*2 read,
and, timed in the same process, the same matrix computed by torch from the stored qkv (softmax(q k^T / 8 + mask), then the mean /
the cast) as the baseline.  Writes profiles/attn_probs_bench.json.  Not a gate: nothing asserts on these numbers.

    python profiles/tools/attn_probs_bench.py [out.json]
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from medvill_amd import hip_ops as ops        # noqa: E402

DEV = "cuda"
A, DH, L = 12, 64, 512
H = A * DH


def timed(fn, reps=200, warm=50, batch=10):
    st = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    nb = max(1, reps // batch)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(nb + 1)]
    evs[0].record(st)
    for i in range(nb):
        for _ in range(batch):
            fn()
        evs[i + 1].record(st)
    evs[-1].synchronize()
    per = [evs[i].elapsed_time(evs[i + 1]) / batch for i in range(nb)]
    return dict(us_median=statistics.median(per) * 1e3, us_min=min(per) * 1e3, us_max=max(per) * 1e3)


def case(B, enc, out_dt, head_mean):
    g = torch.Generator(device=DEV).manual_seed(5)
    qkv = torch.randn((B * L, 3 * H), generator=g, device=DEV).to(enc)
    W, T = (L + 31) // 32, (L + 63) // 64
    bits = torch.zeros((B, L, W), dtype=torch.int32, device=DEV)
    info = torch.zeros((B, T, T), dtype=torch.uint8, device=DEV)
    mask = torch.ones((B, L), dtype=torch.int64, device=DEV)
    mask[:, L - 37:] = 0                                     # a 1-D mask with padding: the last key tile reads its mask words
    ops.mask_pack(mask, bits, info)
    ctx = torch.empty((B * L, H), dtype=enc, device=DEV)
    lse = torch.empty((B, A, L), dtype=torch.float32, device=DEV)
    ops.attn_fwd(qkv, bits, info, ctx, lse, B, L, A, DH)
    out = torch.empty((B, L, L) if head_mean else (B, A, L, L), dtype=out_dt, device=DEV)
    esz = out.element_size()
    nbytes = out.numel() * esz + B * L * 3 * H * 2
    add = ((1 - mask)[:, None, None, :] * -10000.0).float()

    def kernel():
        ops.attn_probs(qkv, bits, info, lse, out, B, L, A, DH, head_mean=head_mean)

    def baseline():
        q, k, _ = (t.view(B, L, A, DH).permute(0, 2, 1, 3) for t in qkv.split(H, dim=-1))
        p = torch.softmax((q @ k.transpose(-1, -2)).float() / 8.0 + add, dim=-1)
        if head_mean:
            p = p.mean(dim=1)
        return p.to(out_dt)

    kernel()
    ref = baseline()
    err = float((out.float() - ref.float()).abs().max())
    tk, tb = timed(kernel), timed(baseline, reps=50, warm=10, batch=5)
    return dict(B=B, L=L, A=A, enc=str(enc), out=str(out_dt), head_mean=bool(head_mean), bytes_model=nbytes, max_abs_diff_vs_torch=err,
                kernel=tk, gbps=nbytes / tk["us_median"] / 1e3, torch_baseline=tb, speedup_vs_torch=tb["us_median"] / tk["us_median"])


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "attn_probs_bench.json")
    rows = []
    for B in (8, 64):
        for out_dt in (torch.float32, torch.float16):
            for hm in (False, True):
                r = case(B, torch.float16, out_dt, hm)
                rows.append(r)
                print(f"B={B:2d} out={str(out_dt):14s} head_mean={int(hm)}  {r['kernel']['us_median']:8.1f} us  {r['gbps']:7.0f} GB/s   torch "
                      f"{r['torch_baseline']['us_median']:8.1f} us  (x{r['speedup_vs_torch']:.1f})  max|d| {r['max_abs_diff_vs_torch']:.1e}", flush=True)
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), scheme="50 warm-up + 200 timed launches in batches of 10, median batch mean (HIP events)",
                       cases=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
