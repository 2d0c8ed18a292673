"""Timing and launch counts of the CMBS event head (csrc/head.hip): forward + backward of ``CMBS(fused=True)`` against the same module with
``fused=False`` (the ATen formulation of the live part), same parameters, same GPU, same run.  Shapes (T, B) = (10, 16) and (10, 128) at
d_model 256, 28 classes; inputs and all eight live parameters require grad, the loss is the sum of the three outputs against fixed
cotangents (``torch.autograd.grad``).
Method: 20 warm-up calls of each, then `--reps` windows of `--inner` calls between two device events, the two formulations ALTERNATING
window by window; reported per call: median (fastest, slowest) window.  ``kernels_faster=yes`` where the kernels' SLOWEST window beats
ATen's FASTEST: those (T, B) are what cmbs._KERNELS_FASTER holds (fused=None takes the kernels there and ATen elsewhere).
Launch counts: afterwards, in windows of their own, torch.profiler counts the device kernels (and, separately, memcpy / memset
operations) of 5 forward + backward calls of each formulation.
usage: python tools/head_bench.py [--reps 9] [--inner 200] [--out profiles/cmbs_head_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgsct_amd  # noqa: E402,F401
from dgsct_amd import CMBS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=200)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("head_bench: needs a GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda:0")
SHAPES = [(10, 16), (10, 128)]
LIVE = ("video_cas", "audio_cas", "localize_module")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


def launches(fn, n=5):
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


say(f"CMBS event head, forward + backward (inputs and the 8 live parameters require grad), fp32, D = 256, K = 28; {torch.cuda.get_device_name(0)}")
say(f"times in us per call: median (fastest, slowest) of {args.reps} windows of {args.inner} calls, the two formulations alternating window by window")
say("fused = CMBS(fused=True): dgsct_cmbs_head_forward + dgsct_cmbs_head_backward;  ATen = the same module with fused=False")
runs = {}
for T, B in SHAPES:
    torch.manual_seed(0)
    mods = {"fused": CMBS(None, fused=True).to(dev), "aten": CMBS(None, fused=False).to(dev)}
    mods["aten"].load_state_dict(mods["fused"].state_dict())
    # inputs at least 1e-5 away from a tie in the top-4 selection and in the arg-max: the two formulations sum in different orders, and a
    # near tie (B = 128 under seed 1: 1.8e-7) makes them select different timesteps, which shows as a gradient difference of a few 1e-2
    mc = mods["aten"].cpu()
    for seed in range(1, 200):
        g = torch.Generator().manual_seed(seed)
        v, a = torch.randn(T, B, 256, generator=g), torch.randn(T, B, 256, generator=g)
        with torch.no_grad():
            s4 = [c.sort(dim=0, descending=True)[0] for c in (mc.video_cas(v), mc.audio_cas(a))]
            sf = ((v + a) / 2).sort(dim=0, descending=True)[0]
            margin = min(min((s[3] - s[4]).min().item() for s in s4), (sf[0] - sf[1]).min().item())
        if margin >= 1e-5:
            break
    else:
        sys.exit("head_bench: no generator seed below 200 gives inputs 1e-5 away from a tie")
    mods["aten"].to(dev)
    v, a = v.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    cots = [torch.randn(T, B, 1, generator=g).to(dev), torch.randn(B, 28, generator=g).to(dev), torch.randn(B, 28, generator=g).to(dev)]
    fns = {}
    for name, m in mods.items():
        wrt = [v, a] + [p for n, p in m.named_parameters() if n.startswith(LIVE)]
        assert len(wrt) == 10
        fns[name] = (lambda m=m, wrt=wrt, v=v, a=a, cots=cots: torch.autograd.grad(list(m(v, a)), wrt, cots))
    ref, got = fns["aten"](), fns["fused"]()
    err = max((x - y).abs().max().item() / max(1.0, x.abs().max().item()) for x, y in zip(ref, got))
    for fn in fns.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ts = {"fused": [], "aten": []}
    for _ in range(args.reps):
        for name in ("fused", "aten"):
            ts[name].append(window(fns[name]))
    f, t = ts["fused"], ts["aten"]
    faster = max(f) < min(t)
    say(f"T={T} B={B} fused {statistics.median(f):.1f} ({min(f):.1f}, {max(f):.1f})  ATen {statistics.median(t):.1f} ({min(t):.1f}, {max(t):.1f})  "
        f"ATen/fused {statistics.median(t) / statistics.median(f):.2f}x  worst gradient difference {err:.1e} (seed {seed}, tie margin {margin:.1e})  kernels_faster={'yes' if faster else 'no'}")
    runs[T, B] = fns
say()
say("launches per forward + backward call (torch.profiler, windows of their own): device kernels, memcpy / memset operations")
for (T, B), fns in runs.items():
    try:
        kf, ka = launches(fns["fused"]), launches(fns["aten"])
        say(f"T={T} B={B} launches: fused {kf[0]:.1f} kernels + {kf[1]:.1f} copies / fills   ATen {ka[0]:.1f} kernels + {ka[1]:.1f} copies / fills")
    except Exception as e:                                   # noqa: BLE001  (a profiler that does not start leaves the timings above standing)
        say(f"T={T} B={B} launches: not measured ({type(e).__name__}: {e})")
say("(the fused count includes what autograd adds around the three kernels: the accumulation of gradients is not part of this call, the "
    "casts / copies of non-contiguous cotangents would be)")
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
