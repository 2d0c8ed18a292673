"""Timing, launch counts and traffic of the audio-visual TPAVI block (csrc/tpavi.hip): three formulations of one ``TPAVIModule`` with the
same parameters on the same GPU in the same run --
  fused      ``fused=True``: the kernels (ops.tpavi), the per-clip setup in torch
  linear     ``fused=False``: the linear form in ATen
  reference  ``reference_order=True``: the reference's order, which materialises f [B, THW, THW]
-- forward alone (no_grad, train mode) and forward + backward (x, audio and the 14 parameters require grad; ``torch.autograd.grad``
against fixed cotangents).  Shapes: B = 4, T = 5, C = 256 at 56^2, 28^2, 14^2, 7^2 (the four decoder scales of AVS-S4), frames layout
``[B*T, C, H, W]`` through ``forward_frames`` as the model calls it.
Method (tools/head_bench.py): warm-up calls of each, then `--reps` windows of `--inner` calls between two device events, the formulations
ALTERNATING window by window; reported per call: median (fastest, slowest) window.  The reference order runs `--inner`/10 calls per window
(at 56^2 one call is 1 TFLOP and 8 GB of f).  ``kernels_faster=yes`` where the kernels' SLOWEST forward + backward window beats the ATen
linear form's FASTEST: those (B*T, H, W) are what tpavi._KERNELS_FASTER holds.
Traffic floor per row: x read once and z written once forward (2 |x| bytes); x and dz read, dx written backward (3 |x|); the achieved
fraction is floor / time against `--peak-tbs` (HBM peak in TB/s, default 8.0).  The kernels' own passes move more than the floor: forward
train reads x twice (statistics, apply); backward reads x three times and moves dr and du through memory once each.
Launch counts: afterwards, in windows of their own, torch.profiler counts the device kernels (and memcpy / memset operations) of 3 calls.
usage: python tools/tpavi_bench.py [--reps 7] [--inner 20] [--out profiles/tpavi_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgsct_amd  # noqa: E402,F401
from dgsct_amd import TPAVIModule  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--peak-tbs", type=float, default=8.0)
ap.add_argument("--sizes", type=int, nargs="*", default=[56, 28, 14, 7])
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tpavi_bench: needs a GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda:0")
B, T, C = 4, 5, 256
NAMES = ("fused", "linear", "reference")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def launches(fn, n=3):
    """(device kernels, memcpy / memset operations) per call, counted by torch.profiler over n calls"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    kern = mem = 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                mem += 1
            else:
                kern += 1
    return kern / n, mem / n


def fmt(ts):
    return f"{statistics.median(ts):.0f} ({min(ts):.0f}, {max(ts):.0f})"


say(f"TPAVI block, fp32, B = {B}, T = {T}, C = {C}, train mode, frames layout [B*T, C, H, W]; {torch.cuda.get_device_name(0)}")
say(f"times in us per call: median (fastest, slowest) of {args.reps} windows of {args.inner} calls ({max(2, args.inner // 10)} for the "
    f"reference order), the formulations alternating window by window; floor fraction against {args.peak_tbs} TB/s")
runs = {}
for S in args.sizes:
    torch.manual_seed(0)
    mods = {"fused": TPAVIModule(C, fused=True), "linear": TPAVIModule(C, fused=False), "reference": TPAVIModule(C, reference_order=True)}
    with torch.no_grad():                                    # the constructor's BatchNorm affine is 0: z = LayerNorm(x); make it live
        mods["fused"].W_z[1].weight.uniform_(0.5, 1.5)
        mods["fused"].W_z[1].bias.uniform_(-0.5, 0.5)
    for n in NAMES:
        mods[n].load_state_dict(mods["fused"].state_dict())
        mods[n].to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * T, C, S, S, generator=g).to(dev).requires_grad_(True)
    audio = torch.randn(B, T, 128, generator=g).to(dev).requires_grad_(True)
    cz, ca = torch.randn(B * T, C, S, S, generator=g).to(dev), torch.randn(B, T, C, generator=g).to(dev)
    xbytes = x.numel() * 4
    fwd, both = {}, {}
    for n, m in mods.items():
        wrt = [x, audio] + list(m.parameters())
        assert len(wrt) == 16

        def f_fwd(m=m, x=x, audio=audio):
            with torch.no_grad():
                return m.forward_frames(x, audio, T=T)
        fwd[n] = f_fwd
        both[n] = (lambda m=m, wrt=wrt, x=x, audio=audio, cz=cz, ca=ca: torch.autograd.grad(list(m.forward_frames(x, audio, T=T)), wrt, [cz, ca]))
    ref, got, lin = both["reference"](), both["fused"](), both["linear"]()
    # one scale for all 16 gradients, the largest |gradient|max of the call: two of them are analytically zero (W_z.0.bias in front of a
    # batch-statistics BatchNorm) and hold only each formulation's own fp32 cancellation noise, which their own scale would magnify
    scale = max(1.0, max(p.abs().max().item() for p in ref))
    err = max((p - q).abs().max().item() for p, q in zip(ref, got)) / scale
    err_l = max((p - q).abs().max().item() for p, q in zip(ref, lin)) / scale
    err_fl = max((p - q).abs().max().item() for p, q in zip(lin, got)) / scale
    del ref, got, lin
    inner = {n: (max(2, args.inner // 10) if n == "reference" else args.inner) for n in NAMES}
    for fns in (fwd, both):
        for n in NAMES:
            for _ in range(3):
                fns[n]()
    torch.cuda.synchronize()
    tf, tb = {n: [] for n in NAMES}, {n: [] for n in NAMES}
    for _ in range(args.reps):
        for n in NAMES:
            tf[n].append(window(fwd[n], inner[n]))
        for n in NAMES:
            tb[n].append(window(both[n], inner[n]))
    faster = max(tb["fused"]) < min(tb["linear"])
    say(f"H=W={S}  |x| = {xbytes / 1e6:.1f} MB")
    for n in NAMES:
        ff = 2 * xbytes / (statistics.median(tf[n]) * 1e-6) / (args.peak_tbs * 1e12)
        fb = 5 * xbytes / (statistics.median(tb[n]) * 1e-6) / (args.peak_tbs * 1e12)
        say(f"  {n:9s} forward {fmt(tf[n])}  floor {2 * xbytes / 1e6:.1f} MB, achieved {ff:.3f}   forward+backward {fmt(tb[n])}  floor "
            f"{5 * xbytes / 1e6:.1f} MB, achieved {fb:.3f}")
    say(f"  linear/fused forward+backward {statistics.median(tb['linear']) / statistics.median(tb['fused']):.2f}x   reference/fused "
        f"{statistics.median(tb['reference']) / statistics.median(tb['fused']):.2f}x   worst gradient difference to the reference order, of the largest gradient's scale: fused "
        f"{err:.1e}, linear {err_l:.1e} (fused to linear {err_fl:.1e})   key ({B * T}, {S}, {S}) kernels_faster={'yes' if faster else 'no'}")
    runs[S] = (fwd, both)
say()
say("launches per call (torch.profiler, windows of their own): device kernels + memcpy / memset operations")
for S, (fwd, both) in runs.items():
    for what, fns in (("forward", fwd), ("forward+backward", both)):
        try:
            say(f"H=W={S} {what}: " + "   ".join("{} {:.1f} + {:.1f}".format(n, *launches(fns[n])) for n in NAMES))
        except Exception as e:                               # noqa: BLE001  (a profiler that does not start leaves the timings above standing)
            say(f"H=W={S} {what}: not measured ({type(e).__name__}: {e})")
say("(fused: 1 frame-sum launch, the torch setup, then 3 launches forward -- statistics, finalise, apply -- and 5 backward -- LayerNorm backward,"
    " row sum, BatchNorm backward + dx, dA / dc, their row sum -- plus the setup's backward and autograd's addition of the broadcast frame-sum "
    "cotangent into dx, the extra pass)")
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
