"""Timing of the patch-merging kernels (csrc/pmerge.hip) at the merges of the AVE trunk, BT = 160: audio (HTS-AT form) 64^2 x 96,
32^2 x 192, 16^2 x 384; visual (Swin-V2 form) 48^2, 24^2, 12^2 maps at the Swin-V2-B widths 128 / 256 / 512 and the Swin-V2-L widths
192 / 384 / 768 -- forward and backward, each against the module's own fused=False ATen formulation on the same GPU in the same run.
Method: 3 warm-up calls, then `--reps` windows of `--inner` calls between two device events; the median window is reported (min / max
beside it).  The backward is timed on its own (`torch.autograd.grad` on a retained graph).  Algorithmic bytes: forward x once in, out once
out; backward dout and x in, dx out; the floor is those bytes at 8 TB/s.
`--train` times the three audio merges as TRAINABLE modules instead (forward + backward with the parameter gradients): the kernels
(fused=True, weight_grads=True) against the formulation AVETrunk(train_htsat=True) runs without that keyword -- both with fp32 master
parameters and a bf16 map, same GPU, same run, same method -- prints what merging._KERNELS_FASTER_TRAIN should hold, and then sets what the parameter gradients add to the frozen
backward beside the GEMM of the route that would materialise its A operand (wgrad_routes).
usage: python tools/patch_merging_bench.py [--batch 160] [--reps 7] [--inner 5] [--train]"""
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
ap.add_argument("--train", action="store_true", help="the audio merges as trainable modules: forward + backward with parameter gradients")
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


def train_bench():
    B = args.batch
    print(f"trainable patch merging (fp32 master parameters, bf16 map), BT = {B}; {torch.cuda.get_device_name(0)}; times in us: median (min, max) "
          f"of {args.reps} windows of {args.inner} calls")
    print("fused = HTSATPatchMerging(fused=True, weight_grads=True): dgsct_patch_merge_forward + dgsct_patch_merge_backward_params;  "
          "ATen = the same module with fused=False")
    print(f"{'merge':<34} {'what':<8} {'fused':>27} {'ATen':>27} {'ATen/fused':>11}")
    listed = []
    for side, C in ((64, 96), (32, 192), (16, 384)):
        torch.manual_seed(0)
        mods = {"fused": HTSATPatchMerging((side, side), C, fused=True, weight_grads=True).to(dev),
                "aten": HTSATPatchMerging((side, side), C, fused=False).to(dev)}
        mods["aten"].load_state_dict(mods["fused"].state_dict())
        x = torch.randn(B, side * side, C, device=dev, dtype=torch.bfloat16, requires_grad=True)
        cot = torch.randn(B, side * side // 4, 2 * C, device=dev, dtype=torch.bfloat16)
        t = {}
        for name, m in mods.items():
            wrt = [x] + list(m.parameters())
            t[name, "fwd"] = timed(lambda: m(x))                                  # (grad mode on: the training forward, what it saves included)
            y = m(x)
            t[name, "bwd"] = timed(lambda: torch.autograd.grad(y, wrt, cot, retain_graph=True))
            del y
            t[name, "fwd+bwd"] = timed(lambda: torch.autograd.grad(m(x), wrt, cot))
        for d in ("fwd", "bwd", "fwd+bwd"):
            f, a = t["fused", d], t["aten", d]
            print(f"audio  HTS-AT    {side:>2}^2 x {C:<4} -> {side // 2:>2}^2 x {2 * C:<4} {d:<8} {f[0]:10.1f} ({f[1]:.1f}, {f[2]:.1f}) {a[0]:10.1f} ({a[1]:.1f}, {a[2]:.1f}) "
                  f"{a[0] / f[0]:10.2f}x", flush=True)
        if t["fused", "fwd+bwd"][2] < t["aten", "fwd+bwd"][1]:                    # the kernels' slowest window against ATen's fastest
            listed.append((mods["fused"]._MODE, side * side, C))
        del mods, x, cot
        torch.cuda.empty_cache()
    print()
    print("forward + backward: the kernels' slowest window faster than ATen's fastest (what merging._KERNELS_FASTER_TRAIN should hold):")
    print("   ", sorted(listed))
    print()
    wgrad_routes()


def wgrad_routes():
    """Raw library calls: what the parameter gradients add to the frozen backward (the column sums, pm_wgrad_k with A staged from the
    map, three memsets), beside the GEMM of the other route -- A [rows, 4C] materialised in bf16 and dout^T . A handed to a library GEMM
    (here torch.mm: hipBLASLt, bf16 out).  That route would ALSO write A (rows x 4C x 2 bytes, not timed here)."""
    from dgsct_amd._lib import PMERGE_NORM_FIRST, default_lib
    from dgsct_amd.merging import gather_2x2
    lib, B, mode = default_lib(), args.batch, PMERGE_NORM_FIRST
    st = torch.cuda.current_stream().cuda_stream
    print("the weight gradient's two routes (raw library calls, NORM_FIRST): backward = dgsct_patch_merge_backward, +params = "
          "dgsct_patch_merge_backward_params;")
    print("materialised = torch.mm(dout^T [2C, rows], A [rows, 4C]) on a bf16 A already in memory: the GEMM alone, without the write of A")
    print(f"{'merge':<34} {'backward':>27} {'+params':>27} {'difference':>11} {'materialised GEMM':>27}")
    for side, C in ((64, 96), (32, 192), (16, 384)):
        torch.manual_seed(0)
        rows = B * side * side // 4
        x = torch.randn(B, side * side, C, device=dev).bfloat16()
        w = (0.05 * torch.randn(2 * C, 4 * C, device=dev)).bfloat16()
        lw, lb = 1 + 0.1 * torch.randn(4 * C, device=dev), 0.1 * torch.randn(4 * C, device=dev)
        out = torch.empty(B, rows // B, 2 * C, device=dev, dtype=torch.bfloat16)
        mu, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        lib.patch_merge_forward(mode, B, side, side, C, x.data_ptr(), w.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, out.data_ptr(), None,
                                mu.data_ptr(), rstd.data_ptr(), st)
        dout, dx = torch.randn_like(out), torch.empty_like(x)
        dw, dlw, dlb = torch.empty(2 * C, 4 * C, device=dev), torch.empty(4 * C, device=dev), torch.empty(4 * C, device=dev)
        ws = torch.empty(lib.patch_merge_params_ws_bytes(mode, B, side, side, C), dtype=torch.uint8, device=dev)
        a = torch.nn.functional.layer_norm(gather_2x2(x, side, side).float(), (4 * C,), lw, lb, 1e-5).bfloat16().reshape(rows, 4 * C)
        dt = dout.reshape(rows, 2 * C).t()
        t0 = timed(lambda: lib.patch_merge_backward(mode, B, side, side, C, dout.data_ptr(), x.data_ptr(), w.data_ptr(), lw.data_ptr(), None,
                                                    mu.data_ptr(), rstd.data_ptr(), 1e-5, dx.data_ptr(), ws.data_ptr(), st))
        t1 = timed(lambda: lib.patch_merge_backward_params(mode, B, side, side, C, dout.data_ptr(), x.data_ptr(), w.data_ptr(), lw.data_ptr(),
                                                           lb.data_ptr(), None, mu.data_ptr(), rstd.data_ptr(), 1e-5, dx.data_ptr(),
                                                           dw.data_ptr(), dlw.data_ptr(), dlb.data_ptr(), ws.data_ptr(), st))
        t2 = timed(lambda: torch.mm(dt, a))
        print(f"audio  HTS-AT    {side:>2}^2 x {C:<4} -> {side // 2:>2}^2 x {2 * C:<4} {t0[0]:10.1f} ({t0[1]:.1f}, {t0[2]:.1f}) {t1[0]:10.1f} ({t1[1]:.1f}, {t1[2]:.1f}) "
              f"{t1[0] - t0[0]:11.1f} {t2[0]:10.1f} ({t2[1]:.1f}, {t2[2]:.1f})", flush=True)
        del x, a, dout, dx, ws
        torch.cuda.empty_cache()


if args.train:
    train_bench()
    sys.exit(0)

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
