"""Timing of the patch-merging kernels (csrc/pmerge.hip) at the merges of the AVE trunk, BT = 160: audio (HTS-AT form) 64^2 x 96,
32^2 x 192, 16^2 x 384; visual (Swin-V2 form) 48^2, 24^2, 12^2 maps at the Swin-V2-B widths 128 / 256 / 512 and the Swin-V2-L widths
192 / 384 / 768 -- forward and backward, each against the module's own fused=False ATen formulation on the same GPU in the same run.
Method: 3 warm-up calls, then `--reps` windows of `--inner` calls between two device events; the median window is reported (min / max
beside it).  The backward is timed on its own (`torch.autograd.grad` on a retained graph).  Algorithmic bytes: forward x once in, out once
out; backward dout and x in, dx out; the floor is those bytes at 8 TB/s.
usage: python tools/patch_merging_bench.py [--batch 160] [--reps 7] [--inner 5]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgsct_amd  # noqa: E402,F401
from dgsct_amd import HTSATPatchMerging, SwinV2PatchMerging  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=160)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("patch_merging_bench: needs a GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda:0")


def timed(fn):
    """(median, min, max) in microseconds per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / args.inner * 1e3)
    return statistics.median(ts), min(ts), max(ts)


CASES = [("audio  HTS-AT   ", HTSATPatchMerging, 64, 96), ("audio  HTS-AT   ", HTSATPatchMerging, 32, 192), ("audio  HTS-AT   ", HTSATPatchMerging, 16, 384),
         ("visual Swin-V2-B", SwinV2PatchMerging, 48, 128), ("visual Swin-V2-B", SwinV2PatchMerging, 24, 256), ("visual Swin-V2-B", SwinV2PatchMerging, 12, 512),
         ("visual Swin-V2-L", SwinV2PatchMerging, 48, 192), ("visual Swin-V2-L", SwinV2PatchMerging, 24, 384), ("visual Swin-V2-L", SwinV2PatchMerging, 12, 768)]
B = args.batch
print(f"patch merging, BT = {B}, bf16; {torch.cuda.get_device_name(0)}; times in us: median (min, max) of {args.reps} windows of {args.inner} calls")
print(f"{'merge':<34} {'dir':<4} {'fused':>24} {'ATen':>24} {'ATen/fused':>11} {'MB':>8} {'floor us':>9} {'of floor':>9}")
slower, faster = [], []
for tag, cls, side, C in CASES:
    torch.manual_seed(0)
    mods = {}
    for name, fused in (("fused", True), ("aten", False)):
        m = cls((side, side), C, fused=fused).to(dev, torch.bfloat16).requires_grad_(False)
        mods[name] = m
    mods["aten"].load_state_dict(mods["fused"].state_dict())
    x = torch.randn(B, side * side, C, device=dev, dtype=torch.bfloat16, requires_grad=True)
    cot = torch.randn(B, side * side // 4, 2 * C, device=dev, dtype=torch.bfloat16)
    by_f = x.numel() * 2 + cot.numel() * 2
    by_b = cot.numel() * 2 + x.numel() * 2 + x.numel() * 2
    t = {}
    for name, m in mods.items():
        with torch.no_grad():
            t[name, "fwd"] = timed(lambda: m(x))
        y = m(x)
        t[name, "bwd"] = timed(lambda: torch.autograd.grad(y, x, cot, retain_graph=True))
        del y
    for d, nb in (("fwd", by_f), ("bwd", by_b)):
        f, a = t["fused", d], t["aten", d]
        floor = nb / 8e6
        print(f"{tag} {side:>2}^2 x {C:<4} -> {side // 2:>2}^2 x {2 * C:<4} {d:<4} {f[0]:9.1f} ({f[1]:.1f}, {f[2]:.1f}) {a[0]:9.1f} ({a[1]:.1f}, {a[2]:.1f}) "
              f"{a[0] / f[0]:10.2f}x {nb / 1e6:8.1f} {floor:9.1f} {floor / f[0]:9.3f}", flush=True)
        if f[0] >= a[0]:
            slower.append((tag.strip(), side, C, d))
    if t["fused", "fwd"][0] < t["aten", "fwd"][0] and t["fused", "bwd"][0] < t["aten", "bwd"][0]:
        faster.append((mods["fused"]._MODE, side * side, C))
    del mods, x, cot
    torch.cuda.empty_cache()
print()
if slower:
    print("fused NOT faster than ATen at:", slower)
print("faster in both directions (what merging._KERNELS_FASTER should hold: fused=None takes the kernels there and ATen elsewhere):")
print("   ", sorted(faster))
