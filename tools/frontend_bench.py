"""Timing of the audio / image front ends (csrc/frontend.hip) at the AVE shapes: 160 waveforms of 320 000 samples -> HTS-AT tokens, and
160 images of 3 x 192 x 192 -> Swin-V2 tokens, each against the module's own fused=False ATen formulation on the same GPU.
Method: 3 warm-up calls, then `--reps` windows of `--inner` calls between two device events; the median window is reported (min / max
beside it).  Traffic floor of the audio path: waveform in, log-mel out and back in, tokens out.
`--train` times the TRAINABLE modules instead (forward + backward with the six / four parameter gradients, fp32 masters, train mode): the
kernels (trainable=True, fused=True: the forward's launches + dgsct_patch_embed_backward_params) against the same module with fused=False,
same GPU, same run, same method, and says what frontend._KERNELS_FASTER_TRAIN should hold.  Traffic floor of the backward: log-mel (or
image) read + dOut read.
`--augment` times the audio front end in train mode with SpecAugment stripes (frontend.draw_stripes, seeded) and a mix-up lambda per
waveform: the kernels (fused=True: dgsct_patch_embed_forward_aug, with `--train` also dgsct_patch_embed_backward_params_aug) against the
fused=False formulation of the SAME augmentation, with the un-augmented rows of the same run beside them, and says whether
frontend._KERNELS_FASTER_AUG should hold the kind measured ("frozen"; with `--train`: "train").
usage: python tools/frontend_bench.py [--batch 160] [--samples 320000] [--reps 7] [--inner 5] [--embed-dim 96] [--train] [--augment]
       (profiles/frontend_bench.txt, profiles/frontend_train_bench.txt and profiles/frontend_aug_bench.txt are its output)"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgsct_amd  # noqa: E402,F401
from dgsct_amd import HTSATFrontEnd, PatchEmbed, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=160)
ap.add_argument("--samples", type=int, default=320000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--embed-dim", type=int, default=96)
ap.add_argument("--train", action="store_true")
ap.add_argument("--augment", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("frontend_bench: needs a GPU (a timing taken elsewhere says nothing)")
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


def row(name, t, nbytes=None):
    med, lo, hi = t
    extra = f"   {nbytes / 1e6:8.1f} MB  {nbytes / med / 1e3:7.0f} GB/s" if nbytes else ""
    print(f"{name:<58} {med:10.1f} us  (min {lo:.1f}, max {hi:.1f}){extra}", flush=True)
    return med


B, L, C = args.batch, args.samples, args.embed_dim
T = L // 320 + 1
gen = torch.Generator().manual_seed(0)
wave = (0.1 * torch.randn(B, L, generator=gen)).to(dev)


def train_rows(tag, mods, x, cot, floor_bytes):
    """fwd / bwd / fwd+bwd of mods = {"fused": ..., "ATen": ...}; returns whether the kernels' slowest fwd+bwd window beat ATen's fastest"""
    res = {}
    for name, m in mods.items():
        params = [q for q in m.parameters() if q.requires_grad]

        def step():
            for q in params:
                q.grad = None
            m(x).backward(cot)

        out = m(x)
        res[name] = (timed(lambda: m(x)), timed(lambda: torch.autograd.grad(out, params, cot, retain_graph=True)), timed(step))
        del out
    for i, what in enumerate(("fwd", "bwd", "fwd+bwd")):
        f, a = res["fused"][i], res["ATen"][i]
        print(f"{tag:<44} {what:<8} {f[0]:9.1f} ({f[1]:.1f}, {f[2]:.1f})   {a[0]:9.1f} ({a[1]:.1f}, {a[2]:.1f})   {a[0] / f[0]:6.2f}x", flush=True)
    bwd = res["fused"][1][0]
    print(f"{tag:<44} backward traffic floor {floor_bytes / 1e6:.1f} MB at 8 TB/s = {floor_bytes / 8e6:.1f} us -> achieved fraction "
          f"{floor_bytes / 8e6 / bwd:.3f}\n", flush=True)
    return res["fused"][2][2] < res["ATen"][2][1]


if args.augment:
    from dgsct_amd import frontend
    kind = "train" if args.train else "frozen"
    stripes = frontend.draw_stripes(B, T, generator=gen)                     # on the host, where a training step draws them
    lam = torch.rand(B, generator=gen).to(dev)
    print(f"augmented audio front end (2 time + 2 mel stripes per waveform, mix-up lambda per waveform; train mode), kind '{kind}': waveform "
          f"[{B}, {L}] -> {T} frames -> tokens [{B}, 4096, {C}]; {torch.cuda.get_device_name(0)}; times in us: median (min, max) of {args.reps} "
          f"windows of {args.inner} calls")
    print("fused = fused=True: the *_aug exports;  ATen = the same module with fused=False (keep mask + torch.flip between bn0 and the stretch)")
    print(f"{'tokens':<8} {'what':<8} {'augmented':<10} {'fused':>28}   {'ATen':>28}   ATen/fused")
    wins = []
    for out_dtype in (torch.bfloat16, torch.float32):
        tag = "bf16" if out_dtype == torch.bfloat16 else "fp32"
        mods = {n: HTSATFrontEnd(embed_dim=C, out_dtype=out_dtype, trainable=args.train, fused=f).to(dev).train() for n, f in (("fused", True), ("ATen", False))}
        cot = torch.randn(B, 4096, C, generator=gen).to(dev, out_dtype)
        res = {}
        for aug in (False, True):
            kw = dict(mixup_lambda=lam, stripes=stripes) if aug else {}
            for name, m in mods.items():
                params = [q for q in m.parameters() if q.requires_grad]

                def step(m=m, params=params, kw=kw):
                    for q in params:
                        q.grad = None
                    m(wave, **kw).backward(cot)

                ts = [timed(lambda m=m, kw=kw: m(wave, **kw))]
                if args.train:
                    out = m(wave, **kw)
                    ts += [timed(lambda out=out, params=params: torch.autograd.grad(out, params, cot, retain_graph=True)), timed(step)]
                    del out
                res[aug, name] = ts
        for i, what in enumerate(("fwd", "bwd", "fwd+bwd") if args.train else ("fwd",)):
            for aug in (False, True):
                f, a = res[aug, "fused"][i], res[aug, "ATen"][i]
                print(f"{tag:<8} {what:<8} {'yes' if aug else 'no':<10} {f[0]:9.1f} ({f[1]:.1f}, {f[2]:.1f})   {a[0]:9.1f} ({a[1]:.1f}, {a[2]:.1f})   "
                      f"{a[0] / f[0]:6.2f}x", flush=True)
        f, a = res[True, "fused"][-1], res[True, "ATen"][-1]
        wins.append(f[2] < a[1])
        print(f"{tag:<8} augmented / un-augmented kernels: {f[0] / res[False, 'fused'][-1][0]:.3f}\n", flush=True)
        del mods, cot, res
        torch.cuda.empty_cache()
    print(f"kind '{kind}': the kernels' slowest augmented window was faster than ATen's fastest in every row (whether "
          f"frontend._KERNELS_FASTER_AUG should hold '{kind}'): {'yes' if all(wins) else 'no'}; it holds {sorted(frontend._KERNELS_FASTER_AUG)}")
    sys.exit(0)

if args.train:
    from dgsct_amd import frontend
    print(f"trainable front end (fp32 master parameters, train mode), batch {B}; {torch.cuda.get_device_name(0)}; times in us: median (min, max) "
          f"of {args.reps} windows of {args.inner} calls")
    print("fused = trainable=True, fused=True: the forward's launches + dgsct_patch_embed_backward_params;  ATen = the same module with fused=False")
    print(f"{'module':<44} {'what':<8} {'fused':>28}   {'ATen':>28}   ATen/fused")
    faster = {"audio": [], "image": []}
    for out_dtype in (torch.bfloat16, torch.float32):
        es = 2 if out_dtype == torch.bfloat16 else 4
        mods = {"fused": HTSATFrontEnd(embed_dim=C, out_dtype=out_dtype, trainable=True, fused=True).to(dev).train(),
                "ATen": HTSATFrontEnd(embed_dim=C, out_dtype=out_dtype, trainable=True, fused=False).to(dev).train()}
        cot = torch.randn(B, 4096, C, generator=gen).to(dev, out_dtype)
        faster["audio"].append(train_rows(f"HTSATFrontEnd [{B}, {L}] -> {'bf16' if es == 2 else 'fp32'} x {C}", mods, wave, cot, B * T * 64 * 4 + B * 4096 * C * es))
        del mods, cot
        torch.cuda.empty_cache()
    del wave
    torch.cuda.empty_cache()
    for Cv in (128, 192):
        img = torch.randn(B, 3, 192, 192, generator=gen).to(dev, torch.bfloat16)
        mods = {"fused": PatchEmbed(192, in_chans=3, embed_dim=Cv, out_dtype=torch.bfloat16, trainable=True, fused=True).to(dev),
                "ATen": PatchEmbed(192, in_chans=3, embed_dim=Cv, out_dtype=torch.bfloat16, trainable=True, fused=False).to(dev)}
        cot = torch.randn(B, 2304, Cv, generator=gen).to(dev, torch.bfloat16)
        faster["image"].append(train_rows(f"PatchEmbed [{B}, 3, 192, 192] bf16 -> bf16 x {Cv}", mods, img, cot, img.numel() * 2 + B * 2304 * Cv * 2))
        del mods, cot, img
        torch.cuda.empty_cache()
    print(f"forward + backward: kinds where the kernels' slowest window was faster than ATen's fastest in every row (what "
          f"frontend._KERNELS_FASTER_TRAIN should hold): {sorted(k for k, v in faster.items() if all(v))}; it holds "
          f"{sorted(frontend._KERNELS_FASTER_TRAIN)}")
    sys.exit(0)

print(f"audio: waveform [{B}, {L}] fp32 -> {T} frames -> tokens [{B}, 4096, {C}]; {torch.cuda.get_device_name(0)}")
for out_dtype in (torch.bfloat16, torch.float32):
    for training in (False, True):
        m = HTSATFrontEnd(embed_dim=C, out_dtype=out_dtype).to(dev).train(training)
        a = HTSATFrontEnd(embed_dim=C, out_dtype=out_dtype, fused=False).to(dev).train(training)
        melW, rng, pe = m.logmel_extractor.melW, m._mel_ranges(), m.patch_embed
        lm = ops.logmel(wave, melW, ranges=rng)
        sc, sh = m._bn_affine(None, None, B * T)
        es = 2 if out_dtype == torch.bfloat16 else 4
        by_lm, by_pe = B * L * 4 + B * T * 64 * 4, B * T * 64 * 4 + B * 4096 * C * es
        tag = f"[{'bf16' if es == 2 else 'fp32'} tokens, {'train' if training else 'eval'}]"
        if training:
            t_lm = row(f"{tag} HIP logmel + statistics (2 launches)", timed(lambda: ops.logmel(wave, melW, want_stats=True, ranges=rng)), by_lm)
        else:
            t_lm = row(f"{tag} HIP logmel (1 launch)", timed(lambda: ops.logmel(wave, melW, ranges=rng)), by_lm)
        t_pe = row(f"{tag} HIP patch_embed, audio mode (1 launch)",
                   timed(lambda: ops.patch_embed(lm, pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias, 1e-5, out_dtype, sc, sh)), by_pe)
        t_f = row(f"{tag} HIP end to end (module call)", timed(lambda: m(wave)), by_lm + by_pe)
        t_a = row(f"{tag} ATen formulation (fused=False), same GPU", timed(lambda: a(wave)))
        print(f"{tag} fused / ATen = {t_f / t_a:.3f}  (ATen / fused = {t_a / t_f:.2f} x);  traffic floor {(by_lm + by_pe) / 1e9:.3f} GB at 8 TB/s = "
              f"{(by_lm + by_pe) / 8e6:.1f} us -> achieved fraction {(by_lm + by_pe) / 8e6 / t_f:.3f}\n", flush=True)
        del m, a, lm
        torch.cuda.empty_cache()

del wave
torch.cuda.empty_cache()
for in_dtype in (torch.bfloat16, torch.float32):
    for Cv in (128, 192):
        img = torch.randn(B, 3, 192, 192, generator=gen).to(dev, in_dtype)
        m = PatchEmbed(192, in_chans=3, embed_dim=Cv, out_dtype=torch.bfloat16).to(dev)
        a = PatchEmbed(192, in_chans=3, embed_dim=Cv, out_dtype=torch.bfloat16, fused=False).to(dev)
        nb = img.numel() * img.element_size() + B * 2304 * Cv * 2
        tag = f"[image {B} x 3 x 192 x 192 {'bf16' if in_dtype == torch.bfloat16 else 'fp32'} -> bf16 tokens, C = {Cv}]"
        t_f = row(f"{tag} HIP", timed(lambda: m(img)), nb)
        t_a = row(f"{tag} ATen", timed(lambda: a(img)))
        print(f"{tag} ATen / fused = {t_a / t_f:.2f} x;  floor at 8 TB/s {nb / 8e6:.1f} us -> achieved fraction {nb / 8e6 / t_f:.3f}\n", flush=True)
