#!/usr/bin/env python
"""Benchmark of the DG-SCT adapter hot path on MI355X (contract: see the task statement / DESIGN.md section 6).

    python bench.py --gpus 1 --steps 20 --warmup 5                       # one GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W         # N GPUs, one rank per GPU (RCCL)

One "step" = the whole AVE adapter stack (48 adapters = 12 layer positions x {p1,p2} x {audio,visual},
reference schedule net_trans.py:880-916) forward + backward on B=16 clips x T=10 frames per GPU of
synthetic feature maps at the BASELINE config-2 shapes (Swin-V2-B + HTS-AT), bf16, followed by the
data-parallel gradient all-reduce (N > 1) and an Adam step on the adapter parameters (the reference
trains them with Adam, main_trans.py:276); weights change every step, so the MFMA-operand weight copies
are re-made every step inside the timed region as well.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times --steps steps and prints the line.  --full adds the diagnostics that take runs of their
own: the host floor, the roofline / per-stage / GEMM-family figures, the CPU baseline and (data-parallel) the all-reduce A/B.
--dump-outputs DIR writes what the last timed step computed (stage outputs, last-stage maps, the updated adapter parameters;
fixed seeded samples of the large ones) as float32 DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import dgsct_amd  # noqa: E402
from dgsct_amd import AdapterStack, GradAllReducer, ave_stage_shapes  # noqa: E402
from dgsct_amd._lib import default_lib  # noqa: E402

MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "bf16_fp8": 2500.0}   # (fp8 products are priced at the bf16 peak: most of the path is bf16)      # dense, MI355X_MICROARCH.md


def alg_flops_per_frame(stages, tk=32, r=8, g=2):
    """F = remap + 8 tk C N + 3 N C^2 + 5 C^2 + N C + 4 N C ds/g per adapter forward per frame."""
    tot = 0.0
    for s in stages:
        for (N, C, No, Co) in ((s["Nv"], s["Cv"], s["Na"], s["Ca"]), (s["Na"], s["Ca"], s["Nv"], s["Cv"])):
            remap = min(2 * N * No * Co + 2 * N * Co * C, 2 * No * Co * C + 2 * N * No * C)
            f = remap + 8 * tk * C * N + 3 * N * C * C + 5 * C * C + N * C + 4 * N * C * (C // r) // g
            tot += f * 2 * s["layers"]            # p1 + p2
    return tot


def alg_bytes_per_step(stages, BT, es=2):
    """per adapter per frame fwd es*(2NC + NoCo + N), bwd es*(3NC + 2NoCo); + 3 x 4 B per parameter per step."""
    tot = 0.0
    for s in stages:
        for (N, C, No, Co) in ((s["Nv"], s["Cv"], s["Na"], s["Ca"]), (s["Na"], s["Ca"], s["Nv"], s["Cv"])):
            tot += (es * (2 * N * C + No * Co + N) + es * (3 * N * C + 2 * No * Co)) * 2 * s["layers"] * BT
            nparam = N * No + C * Co + 2 * C * C + 3 * (C // 2) * C + C * (C // 2) + 2 * C * (C // 8) // 2 + 32 * C
            tot += 3 * 4 * nparam * 2 * s["layers"]
    return tot


def build_stack(backbone, dtype, device, concurrent=True, fp8=False, num_tokens=32):
    torch.manual_seed(0)
    stages = ave_stage_shapes(backbone)
    from dgsct_amd.stack import default_opt
    stack = AdapterStack(stages, opt=default_opt(num_tokens=num_tokens), compute_dtype=dtype, concurrent=concurrent, fp8_projections=fp8).to(device)
    with torch.no_grad():              # BEFORE flattening: afterwards the per-name tensors are views, not parameters
        for n, p in stack.named_parameters():
            if n.endswith("gate") or n.endswith("gate_av"):
                p.fill_(0.5)                       # default 0 makes the path degenerate
    stack.flatten_parameters()         # one flat fp32 parameter (and one flat gradient) per adapter: 48 tensors, not ~1900
    for m in stack.modules():
        if hasattr(m, "_flat_views"):
            assert float(m._flat_views["gate_av"]) == 0.5 and float(m._flat_views["gate"]) == 0.5
    return stages, stack


def make_inputs(stages, BT, dtype, device, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    feats, cots = [], []
    for s in stages:
        fv = torch.randn(BT, s["Nv"], s["Cv"], generator=gen).to(device=device, dtype=dtype).requires_grad_(True)
        fa = torch.randn(BT, s["Na"], s["Ca"], generator=gen).to(device=device, dtype=dtype).requires_grad_(True)
        feats.append((fv, fa))
        cots.append((torch.randn(BT, s["Nv"], s["Cv"], generator=gen).to(device=device, dtype=dtype),
                     torch.randn(BT, s["Na"], s["Ca"], generator=gen).to(device=device, dtype=dtype)))
    s = stages[-1]
    mcots = (torch.randn(BT, 1, s["Nv"], generator=gen).to(device), torch.randn(BT, 1, s["Na"], generator=gen).to(device))
    return feats, cots, mcots


def stage_breakdown(lib, stages, run_step, BT, peak_tflops, nsteps=2):
    """Where the step is: per backbone stage, the wall span of its adapter calls inside the REAL schedule (both
    adapter streams + aux streams; the library records an event pair around every forward / backward call on the call's own stream:
    dgsct_test_tune("callprof"), no tracer), the stage's algorithmic FLOPs and the fraction of the dense MFMA peak."""
    import tempfile
    path = os.path.join(tempfile.gettempdir(), f"dgsct_callprof_{os.getpid()}.txt")
    old_env = os.environ.get("DGSCT_CALL_PROF")
    os.environ["DGSCT_CALL_PROF"] = path
    by_n = {}
    for i, st in enumerate(stages):
        by_n[(st["Nv"], st["Cv"])] = i
        by_n[(st["Na"], st["Ca"])] = i
    acc = [[0.0, 0.0] for _ in stages]
    try:
        for _ in range(nsteps):
            lib.test_tune("callprof", 1)
            run_step()
            torch.cuda.synchronize()
            lib.test_tune("callprof", 0)
            lib.test_tune("callprof", 2)                       # dump + clear
            spans = {}
            for ln in open(path):
                kind, N, C, _, a, b = ln.split()
                i = by_n.get((int(N), int(C)))
                if i is None:
                    continue
                e = spans.setdefault((i, kind), [float("inf"), 0.0])
                e[0] = min(e[0], float(a)); e[1] = max(e[1], float(b))
            for (i, kind), (a, b) in spans.items():
                acc[i][0 if kind == "fwd" else 1] += (b - a) * 1e-3
    finally:
        if old_env is None:
            os.environ.pop("DGSCT_CALL_PROF", None)
        else:
            os.environ["DGSCT_CALL_PROF"] = old_env
        try:
            os.remove(path)
        except OSError:
            pass
    out = []
    for i, st in enumerate(stages):
        f, b = acc[i][0] / nsteps, acc[i][1] / nsteps
        tf = 3.0 * alg_flops_per_frame([st]) * BT / 1e12
        out.append(dict(stage=i, adapter_calls=4 * st["layers"], fwd_ms=round(f, 3), bwd_ms=round(b, 3), ms=round(f + b, 3),
                        alg_tflop=round(tf, 3), frac_of_mfma_peak=round(tf / ((f + b) * 1e-3) / peak_tflops, 4) if f + b > 0 else None))
    return out


def cpu_baseline(backbone, max_seconds=30.0, b16_seconds=45.0):
    """The oracle's autograd 'port' (op-for-op ATen restatement of the reference adapter, token-major) timed on the
    host cores: ONE clip (BT = 10 frames) through all 48 adapters, forward + backward, fp32."""
    from oracle import dgsct_oracle as O
    stages = ave_stage_shapes(backbone)
    BT = 10
    torch.manual_seed(0)
    adapters = []
    for s in stages:
        for (N, C, No, Co) in ((s["Na"], s["Ca"], s["Nv"], s["Cv"]), (s["Nv"], s["Cv"], s["Na"], s["Ca"])):
            cfg = O.AdapterConfig(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2)
            for _ in range(2 * s["layers"]):
                p = O.random_params(cfg, "ave", seed=len(adapters))
                p = {k: (v.requires_grad_(True) if v.is_floating_point() and "running" not in k and not k.startswith("_") else v)
                     for k, v in p.items()}
                adapters.append((cfg, p))

    def one_pass():
        t0 = time.perf_counter()
        for cfg, p in adapters:
            X = torch.randn(BT, cfg.N, cfg.C, requires_grad=True)
            Y = torch.randn(BT, cfg.No, cfg.Co, requires_grad=True)
            out, amap, _ = O.forward_autograd(p, X, Y, cfg, training=True)
            torch.autograd.backward([out, amap], [torch.randn_like(out), torch.randn_like(amap)])
            for v in p.values():
                if v.requires_grad:
                    v.grad = None
        return time.perf_counter() - t0

    # pick the intra-op thread count that serves this op mix best on this host (all logical CPUs is rarely it)
    ncpu = os.cpu_count() or 1
    best_n, best_t = torch.get_num_threads(), None
    probe = [a for a in adapters if a[0].N in (144, 256)][:2]
    for n in sorted({min(ncpu, c) for c in (8, 16, 32, 64, ncpu)}):
        torch.set_num_threads(n)
        full, adapters[:] = adapters[:], probe
        one_pass()
        t = one_pass()
        adapters[:] = full
        if best_t is None or t < best_t:
            best_n, best_t = n, t
    torch.set_num_threads(best_n)

    t_warm = one_pass()
    times = []
    budget = max_seconds / 2 - t_warm
    while budget > 0 and len(times) < 3:
        t = one_pass()
        times.append(t)
        budget -= t
    if not times:
        times = [t_warm]
    t = sorted(times)[len(times) // 2]

    # B = 16 (the batch the GPU number is quoted on; SURVEY.md 8d: "B=16 ... fall back to per-stage timing and sum"): ONE
    # forward+backward of each of the 8 distinct adapter shapes at BT = 160, scaled by how often the stack runs that shape --
    # about a fifth of a full 48-adapter pass of CPU work (a full pass holds ~40 GB of saved activations and takes ~30 s)
    t16, n16, cold16 = 0.0, 0, 0
    seen = {}
    for cfg, p in adapters:
        key = (cfg.N, cfg.C, cfg.No, cfg.Co)
        seen.setdefault(key, [cfg, p, 0])[2] += 1
    # its OWN budget (round 4's driver line lost this leg to the B=1 leg's clock): one warm-up pass + one timed pass per shape while
    # the budget lasts, then ONE (cold, timed) pass per remaining shape -- the leg always completes, `cold_shapes` says how
    t_budget = time.perf_counter() + b16_seconds
    for key, (cfg, p, cnt) in seen.items():
        X = torch.randn(160, cfg.N, cfg.C, requires_grad=True)
        Y = torch.randn(160, cfg.No, cfg.Co, requires_grad=True)
        dts = []
        for rep in range(2):              # warm-up pass (first touch of the multi-GB saved activations), then the timed one
            go, gm = torch.randn(160, cfg.N, cfg.C), torch.randn(160, 1, cfg.N)
            t0 = time.perf_counter()
            out, amap, _ = O.forward_autograd(p, X, Y, cfg, training=True)
            torch.autograd.backward([out, amap], [go.reshape(out.shape), gm.reshape(amap.shape)])
            dt = time.perf_counter() - t0
            for v in p.values():
                if v.requires_grad:
                    v.grad = None
            X.grad = Y.grad = None
            del out, amap
            dts.append(dt)
            if time.perf_counter() + dt > t_budget:
                break
        del X, Y
        cold16 += len(dts) == 1
        t16 += cnt * dts[-1]
        n16 += 1
    model = "unknown"
    physical = None
    try:
        cores = set()
        phys_id = core_id = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys_id = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core_id = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys_id is not None and core_id is not None:
                    cores.add((phys_id, core_id))
                phys_id = core_id = None
        physical = len(cores) or None
    except OSError:
        pass
    b1 = round(1.0 / t, 4)
    b16 = round(16.0 / t16, 4) if t16 else None
    return dict(value=b16 if b16 is not None else b1, unit="clips/s", cores=torch.get_num_threads(), kind="port", cpu_model=model,
                logical_cpus=ncpu, physical_cores=physical, value_b1=b1, value_b16=b16, b16_cold_shapes=cold16,
                # a shape timed on its single cold pass (first touch of multi-GB buffers) makes the CPU look slower than it is: the
                # GPU / CPU ratio of such a line is an upper bound
                value_is_lower_bound=bool(cold16),
                sample=(f"B=16: fwd+bwd of each of the {n16} distinct adapter shapes at BT=160 (one warm-up pass + one timed pass; {cold16} shape(s) timed cold "
                        f"once the leg's own {b16_seconds:.0f} s budget ran out), weighted by the stack's call "
                        f"counts (= {t16:.1f} s for the 48-adapter step; `value`); ") +
                       f"B=1: 1 clip (BT=10) x 48 adapters, median of {len(times)} passes after 1 warm-up ({t:.2f} s/pass; `value_b1`).  "
                       f"fp32, oracle.forward_autograd (ATen op-for-op port of the reference adapter on token-major maps: at least as fast "
                       f"as the reference's permuted-view path), thread count picked by a sweep")


DUMP_OUT_ELEMS = 1 << 20          # per stage-output array (8 of them: 32 MB)
DUMP_PARAM_ELEMS = 1 << 15        # per adapter parameter tensor (96 of them: at most 12.6 MB)


def _sample(t, n, seed):
    """float32 numpy copy of t (flattened), or of a fixed seeded sample of n of its elements (sorted indices)."""
    import numpy as np
    flat = t.detach().reshape(-1)
    if flat.numel() > n:
        idx = np.sort(np.random.default_rng(seed).choice(flat.numel(), n, replace=False))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.float().cpu().numpy()


def dump_outputs(path, outs, maps, params):
    """What the last timed step hands back to its caller: the stage outputs (f_v, f_a) and the last stage's maps of the forward,
    and the adapter parameters after the optimizer step."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {}
    for s, (fv, fa) in enumerate(outs):
        arrays[f"out_stage{s}_visual"] = _sample(fv, DUMP_OUT_ELEMS, [s, 0])
        arrays[f"out_stage{s}_audio"] = _sample(fa, DUMP_OUT_ELEMS, [s, 1])
    arrays["map_visual"] = _sample(maps[0], DUMP_OUT_ELEMS, [99, 0])
    arrays["map_audio"] = _sample(maps[1], DUMP_OUT_ELEMS, [99, 1])
    arrays["params"] = np.concatenate([_sample(p, DUMP_PARAM_ELEMS, [i, 2]) for i, p in enumerate(params)])
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16, help="clips per GPU (T=10 frames each)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --batch clips on EVERY GPU (the driver's default); strong: --batch is the GLOBAL batch (BASELINE's fixed "
                         "B=16), split over the ranks (must divide)")
    ap.add_argument("--backbone", default="swinv2_base", choices=["swinv2_base", "swinv2_large"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16_fp8"],
                    help="bf16_fp8: bf16 storage with e4m3 MFMA operands for the three weight-stationary forward projections (BASELINE configs[4]); "
                         "the backward products stay bf16 (a straight-through estimate, tests/test_fp8.py)")
    ap.add_argument("--blocks", action="store_true", help="harness B (SURVEY.md 8d / row f4): the frozen Swin-V2 half-blocks and HTS-AT blocks "
                    "(dgsct_amd/backbone.py, random-init, frozen, PyTorch-ROCm ops) inside the layer loop -- NOT the graded workload; the line "
                    "says so in config.workload")
    ap.add_argument("--full", action="store_true", help="also the diagnostics beyond the headline: host floor, roofline / per-stage figures, "
                    "CPU baseline, data-parallel all-reduce A/B (each can still be left out with its --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--num-tokens", type=int, default=32, help="latent tokens per adapter (every reference launcher: <= 32 = the graded "
                    "workload; more -- the reference constructor's default is 87 -- runs the attentions on csrc/attn_wide.cpp)")
    ap.add_argument("--no-optim", action="store_true", help="time fwd+bwd(+all-reduce) only")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--serial", action="store_true", help="one HIP stream (no audio/visual adapter overlap)")
    ap.add_argument("--no-aux", action="store_true", help="no aux stream for weight gradients")
    ap.add_argument("--force-dp", action="store_true", help="run the RCCL gradient all-reduce path even with one rank (self-test)")
    ap.add_argument("--no-overlap", action="store_true", help="DP: one grouped all-reduce after backward instead of per-stage "
                    "buckets launched from autograd hooks while the earlier stages' backward still runs (DESIGN.md section 5)")
    ap.add_argument("--phases", action="store_true", help="also report GPU ms of forward / backward (events on the main stream)")
    ap.add_argument("--graph", action="store_true", help="replay one captured HIP graph per step instead of eager launches "
                    "(ROCm 7.2: replaying ~6000 nodes costs as much host time as launching them, so this is off by default)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    dp = world > 1 or args.force_dp
    if dp:
        import torch.distributed as dist
        if "RANK" not in os.environ:       # --force-dp without a launcher
            os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29531")
        from dgsct_amd import init_process_group
        init_process_group(device)       # "nccl" IS RCCL on ROCm (one process per GPU, bound to its device)
    dtype = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    fp8 = args.dtype == "bf16_fp8"
    T = 10
    per_gpu_batch = args.batch
    if args.scaling == "strong":
        if args.batch % world:
            raise SystemExit(f"--scaling strong: the global batch {args.batch} is not divisible by {world} ranks")
        per_gpu_batch = args.batch // world                 # clips of the fixed global batch that land on this rank
    BT = per_gpu_batch * T

    stages, stack = build_stack(args.backbone, dtype, device, concurrent=not args.serial, fp8=fp8, num_tokens=args.num_tokens)
    stack.train()
    params = [p for p in stack.parameters() if p.requires_grad]
    if dp:
        import torch.distributed as dist
        for p in stack.parameters():
            dist.broadcast(p.data, 0)
    # N > 1: the 48 flat gradient buffers are all-reduced in place (RCCL, ncclAvg) as ONE grouped call after backward.
    # --overlap launches per-stage groups from autograd hooks instead; on ROCm 7.2 its extra cross-stream events can
    # stall the HIP launch path depending on stream->hardware-queue placement, so it is opt-in.
    reducer = GradAllReducer(GradAllReducer.stage_buckets(stack), overlap=(not args.no_overlap) and not args.graph, force=args.force_dp) if dp else None
    use_graph = args.graph
    if use_graph or args.no_aux:
        from dgsct_amd import ops as _ops
        _ops.USE_AUX_STREAM = False        # event fork/join from inside the library is not capture-safe on ROCm 7.2
    opt = None
    if not args.no_optim:
        try:        # one fused multi-tensor Adam launch per dtype/device group instead of ~10 foreach launches
            opt = torch.optim.Adam(params, lr=1e-5, fused=True, capturable=use_graph)
        except Exception:
            opt = torch.optim.Adam(params, lr=1e-5, capturable=use_graph)
    feats, cots, mcots = make_inputs(stages, BT, dtype, device, seed=1 + rank)

    phase_ev = []                          # (start, end-of-forward, end-of-backward) events of the timed steps (--phases)
    last = []                              # the forward results of the latest step, detached (--dump-outputs)
    from dgsct_amd.train import StackTrainer
    trainer = StackTrainer(stack, opt, reducer)      # the step logic the gloo world-2 test drives (tests/test_host_cpu.py)
    if args.blocks:
        from dgsct_amd import FrozenBlocks
        fb = FrozenBlocks(stages, dtype=dtype).to(device)
        trainer.block_kwargs = dict(vis_block=fb.vis_block_map, aud_block=fb.aud_block)

    def fwd_bwd():
        if args.phases:
            e0 = torch.cuda.Event(enable_timing=True); e0.record()
            outs, maps = stack(feats, **getattr(trainer, "block_kwargs", {}))
            e1 = torch.cuda.Event(enable_timing=True); e1.record()
            torch.autograd.backward([t for pair in outs for t in pair] + [maps[0], maps[1]],
                                    [g for pair in cots for g in pair] + [mcots[0], mcots[1]])
            e2 = torch.cuda.Event(enable_timing=True); e2.record()
            phase_ev.append((e0, e1, e2))
            for fv, fa in feats:
                fv.grad = None
                fa.grad = None
        else:
            outs, maps = trainer.fwd_bwd(feats, cots, mcots)
        last[:] = [[(fv.detach(), fa.detach()) for fv, fa in outs], (maps[0].detach(), maps[1].detach())]

    def update():
        if opt is not None:
            opt.step()
        trainer.zero_grad(set_to_none=not (use_graph and dp))

    graphs = []

    def capture(fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs.append(g)
        return g.replay

    host_parts = [0.0, 0.0, 0.0]           # host seconds spent enqueueing fwd+bwd / all-reduce / optimizer

    def eager_step():
        t0 = time.perf_counter()
        fwd_bwd()
        t1 = time.perf_counter()
        if reducer is not None:
            reducer.finish()
        t2 = time.perf_counter()
        update()
        t3 = time.perf_counter()
        host_parts[0] += t1 - t0
        host_parts[1] += t2 - t1
        host_parts[2] += t3 - t2

    step = eager_step
    if use_graph:
        # One HIP graph per step: ~6000 kernel launches (48 adapters x ~125 kernels) replayed with a single
        # hipGraphLaunch, so the host is out of the critical path (eager: ~100 ms of host enqueue per step).
        s = torch.cuda.Stream(device=device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s):
            for _ in range(2):
                eager_step()            # allocator + optimizer-state warm-up, as torch.cuda.graphs requires
        torch.cuda.current_stream(device).wait_stream(s)
        torch.cuda.synchronize()
        if not dp:
            def whole():
                fwd_bwd()
                update()
            step = capture(whole)
        else:
            for p in params:            # static .grad buffers: backward accumulates into them inside the graph
                p.grad = torch.zeros_like(p) if p.grad is None else p.grad.zero_()
            g_fb = capture(fwd_bwd)

            def step():
                g_fb()
                reducer.finish()
                update()                # zero_grad(set_to_none=False): keeps the captured buffers

    def barrier():
        if dp:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    host_parts[:] = [0.0, 0.0, 0.0]
    t0 = time.perf_counter()
    host_s = 0.0
    for _ in range(args.steps):
        h0 = time.perf_counter()
        step()
        host_s += time.perf_counter() - h0
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed_local = elapsed
    if dp:
        import torch.distributed as dist
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    ms_per_step = elapsed / args.steps * 1e3
    host_ms = [round(x / args.steps * 1e3, 2) for x in host_parts]
    clips_per_s = per_gpu_batch * world / (elapsed / args.steps)
    if args.dump_outputs and rank == 0:          # before the --full legs: they run further steps
        dump_outputs(args.dump_outputs, last[0], last[1], params)

    roofline_leg = args.full and not args.no_roofline
    host_floor = None
    if rank == 0 and world == 1 and not use_graph and roofline_leg:
        # What the HOST needs per step: the same step on ONE clip (BT = 10: a sixteenth of the device work, every
        # launch still issued) is enqueue-bound -- its wall time per step is the host's floor for this schedule: Python + autograd +
        # ctypes + the library's launches and event forks.  Not part of `value`.
        try:
            f1, c1, m1 = make_inputs(stages, T, dtype, device, seed=99)

            def small_step():
                trainer.fwd_bwd(f1, c1, m1)
                update()
            for _ in range(2):
                small_step()
            torch.cuda.synchronize()
            tq = time.perf_counter()
            nq = 5
            for _ in range(nq):
                small_step()
            torch.cuda.synchronize()
            host_floor = round((time.perf_counter() - tq) / nq * 1e3, 2)
            del f1, c1, m1
        except Exception as ex:                          # diagnostics only
            host_floor = None

    roofline = None
    if rank == 0 and roofline_leg:
        # dominant kernel family = the MFMA GEMM engine (gemm_kernel<...>): time every launch of two extra steps
        # with HIP events on the launch stream (the library records them itself: dgsct_prof_enable).
        lib = default_lib()
        from dgsct_amd import ops as _ops
        conc, aux = stack.concurrent, _ops.USE_AUX_STREAM
        stack.concurrent, _ops.USE_AUX_STREAM = False, False      # one stream: a kernel's events then bracket that kernel alone

        def local_step():                # rank-local (no collective: the other ranks are not in this pass)
            fwd_bwd()
            update()

        if reducer is not None:
            reducer.paused = True        # the autograd hooks must not launch collectives here

        local_step()
        torch.cuda.synchronize()
        lib.prof_enable(True)
        nprof = 2
        for _ in range(nprof):
            local_step()                 # eager launches: the library brackets each GEMM launch with HIP events
        torch.cuda.synchronize()
        import csv
        import tempfile
        keep_dump = "DGSCT_PROF_DUMP" in os.environ       # (kept when the caller asked for the per-launch log)
        dump = os.environ.get("DGSCT_PROF_DUMP") or os.path.join(tempfile.gettempdir(), f"dgsct_gemm_prof_{os.getpid()}.csv")
        os.environ["DGSCT_PROF_DUMP"] = dump            # the library also writes one line per launch (shape, ms)
        launches, gemm_ms, gemm_flops = lib.prof_collect()
        if not keep_dump:
            os.environ.pop("DGSCT_PROF_DUMP", None)
        lib.prof_enable(False)
        heaviest = None
        try:                                            # the single heaviest launch shape of the family (by time)
            by_shape = {}
            for r in csv.DictReader(open(dump)):
                key = (r["M"], r["N"], r["K"], r["KB"], r["batch"], r["ak"], r["bk"], r["atomic"])
                a = by_shape.setdefault(key, [0, 0.0, 0.0])
                a[0] += 1; a[1] += float(r["ms"]); a[2] += float(r["flops"])
            key, (cnt, ms, fl) = max(by_shape.items(), key=lambda kv: kv[1][1])
            heaviest = dict(shape=dict(M=int(key[0]), N=int(key[1]), K=int(key[2]), K_frames=int(key[3]), batch=int(key[4]),
                                       a_kmajor=int(key[5]), b_kmajor=int(key[6]), split_k_atomic=int(key[7])),
                            launches_per_step=cnt // nprof, avg_launch_us=round(ms / cnt * 1e3, 1),
                            achieved=round(fl / (ms * 1e-3) / 1e12, 1), frac=round(fl / (ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[args.dtype], 4),
                            share_of_gemm_time=round(ms / gemm_ms, 3))
            if not keep_dump:
                os.remove(dump)
        except Exception:
            pass
        stack.concurrent, _ops.USE_AUX_STREAM = conc, aux
        per_stage = None
        try:                                            # the step's own (concurrent) schedule again, with per-call event pairs
            per_stage = stage_breakdown(lib, stages, local_step, BT, MFMA_PEAK_TFLOPS[args.dtype])
        except Exception as ex:                         # diagnostics only: never lose the bench line over it
            per_stage = dict(error=str(ex))
        if reducer is not None:
            reducer.paused = False
        alg = 3.0 * alg_flops_per_frame(stages, tk=args.num_tokens) * BT                 # fwd + bwd, per step
        peak = MFMA_PEAK_TFLOPS[args.dtype]
        # the GEMM family's own useful FLOPs (2 M N K per launch, summed by the library) over its own time: the latent-token
        # attention products (8 tk C N per frame of the algorithmic count) now run in the fused attention kernels, not here
        achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        traffic = None
        step_block = dict(frac_of_mfma_peak=round(alg / (ms_per_step * 1e-3) / 1e12 / peak, 4), alg_gb_per_step=round(alg_bytes_per_step(stages, BT) / 1e9, 2))
        try:        # what the 48 forward calls of a step keep for their backward (dgsct_query: `saved`) and the scratch of one call
            from dgsct_amd import ops as _o
            sv = wsb = 0
            for m in stack.modules():
                if hasattr(m, "spec") and hasattr(m.spec, "desc"):
                    sz = lib.query(m.spec.desc(BT, dtype, True))
                    sv += int(sz.saved_bytes); wsb = max(wsb, int(sz.ws_bwd_bytes))
            step_block.update(saved_gb_per_step=round(sv / 1e9, 2), largest_bwd_workspace_gb=round(wsb / 1e9, 2))
        except Exception:
            pass
        import glob
        tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
        tsrc = None
        if tfiles and args.backbone == "swinv2_base" and per_gpu_batch == 16 and args.dtype == "bf16":
            # bytes through the L2's memory-side port (FETCH_SIZE x2 + WRITE_SIZE; separate rocprofv3 --pmc passes over the 8
            # adapter shapes of this exact workload, scaled by the schedule: tools/pmc_stack.sh + pmc_stack_summary.py)
            tj = json.load(open(tfiles[-1]))
            tsrc = os.path.relpath(tfiles[-1], ROOT)
            traffic = round(tj["gemm_kernel<*>"]["bytes_per_launch"])
            if "_total" in tj:
                tb = tj["_total"]["bytes"]
                step_block.update(pmc_gb_per_step=round(tb / 1e9, 1), pmc_over_alg=round(tb / alg_bytes_per_step(stages, BT), 2),
                                  hbm_side_gbps=round(tb / 1e9 / (ms_per_step * 1e-3)), frac_of_hbm_peak=round(tb / (ms_per_step * 1e-3) / 8e12, 3))
                # which roof is closer: the step as a whole is limited by memory-side traffic of its multi-pass schedule
                step_block["bound_by_data"] = "hbm" if step_block["frac_of_hbm_peak"] > step_block["frac_of_mfma_peak"] else "mfma"
        # the same family INSIDE the timed schedule (two adapter streams + aux streams, kernels overlapping each other): its
        # summed duration from a rocprofv3 --kernel-trace of this command, committed under profiles/ by tools/profile_round.sh
        in_step = None
        gfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_in_step.json")))
        if gfiles and args.backbone == "swinv2_base" and per_gpu_batch == 16 and args.dtype == "bf16":
            gj = json.load(open(gfiles[-1]))
            if gj.get("gemm_ms_per_step"):
                in_step = dict(frac=round(gemm_flops / nprof / (gj["gemm_ms_per_step"] * 1e-3) / 1e12 / peak, 4), gemm_ms_per_step=gj["gemm_ms_per_step"],
                               launches_per_step=gj.get("launches_per_step"), source=os.path.relpath(gfiles[-1], ROOT))
        # ---- one set of books.  The family is {gemm_kernel, gemm8_kernel, gemm_fx_kernel, wgrad_bt_k}: the launch count,
        # the traffic per launch and the algorithmic bytes per launch all use the launch count of the committed trace / PMC passes of
        # this command (same family definition in tools/rocpd_stats.py and tools/pmc_stack_summary.py); the library's own event log counts
        # the skinny / tall products as well and is kept as `launches_logged`.  The HEADLINE fraction is the one inside the timed
        # two-stream schedule (trace); the serial-pass figure (each launch alone between its own events) is `frac_serial`.
        fam_launches = int(in_step["launches_per_step"]) if in_step and in_step.get("launches_per_step") else launches // nprof
        frac_head = in_step["frac"] if in_step else round(achieved / peak, 4)
        ach_head = round(frac_head * peak, 2)
        row_kernels = None
        if tsrc:
            # the HBM-bound kernels individually ("the purely elementwise / normalisation kernels ... HBM fraction when
            # profiled individually"): PMC bytes (FETCH x2 + WRITE) over the kernel's own duration in the same per-shape passes
            row_kernels = {}
            for k in ("tail_fwd_k", "tail_bwd_ave_k", "modln_fwd_k", "modln_bwd_k", "gatemod_fwd_k", "gatemod_bwd_k", "vq1_bwd_k", "xattn_fwd2_k",
                      "xattn_bwd2_k", "xattn_fwd3_k", "xattn_bwd3_k", "tokattn_fwd_k", "tokattn_fwd_small_k", "tokattn_bwd_k", "tokattn_bwd2_k",
                      "gproj_narrow_k", "gproj_wide_k", "gemm_tall_k", "scale_cols_k", "relu_bwd_scale_k"):
                e = tj.get(k)
                if e and e.get("serial_ms"):
                    gbs = (e["fetch_bytes"] + e["write_bytes"]) / 1e9 / (e["serial_ms"] * 1e-3)
                    row_kernels[k] = dict(launches_per_step=e["launches_per_step"], ms_per_step_alone=round(e["serial_ms"], 3),
                                          mb_per_launch=round(e["bytes_per_launch"] / 1e6, 1), achieved_gbps=round(gbs), frac_of_hbm_peak=round(gbs / 8000.0, 3))
        roofline = dict(bound="mfma", achieved=ach_head, peak=peak, unit="TFLOP/s", frac=frac_head,
                        frac_serial=round(achieved / peak, 4), frac_in_step=in_step["frac"] if in_step else None, in_step=in_step,
                        traffic=traffic, traffic_unit=f"bytes/launch (PMC, {tsrc}; family bytes / {fam_launches} launches)" if tsrc else None,
                        traffic_source=("committed: separate rocprofv3 --pmc passes over this workload's 8 adapter shapes "
                                        "(tools/pmc_stack.sh), not measured in this run") if tsrc else None,
                        alg_bytes_per_launch=round(alg_bytes_per_step(stages, BT) / max(fam_launches, 1)), kernel="dgsct::gemm_kernel<*> + gemm8_kernel<*> + gemm_fx_kernel<*> + wgrad_bt_k (the MFMA GEMM family of a step)",
                        launches_per_step=fam_launches, launches_logged=launches // nprof, avg_launch_us=round(gemm_ms * 1e3 / max(launches, 1), 2),
                        alg_tflop_per_step=round(alg / 1e12, 3), executed_tflop_per_step=round(gemm_flops / nprof / 1e12, 3),
                        gemm_ms_per_step=round(gemm_ms / nprof, 3), heaviest_launch=heaviest,
                        step_frac_of_mfma_peak=step_block["frac_of_mfma_peak"], step=step_block, per_stage=per_stage, row_kernels=row_kernels)
    dp_info = None
    if dp and args.full:
        # what a driver log needs to diagnose a multi-GPU run without a second one: ranks RCCL really has, buckets launched from
        # the hooks, the spread of the per-rank step time, and the EXPOSED cost of the gradient exchange = this step against the
        # same steps with the exchange switched off (A/B inside this run, after the timed region; weights diverge, nothing reads them)
        import torch.distributed as dist
        barrier()
        mine = torch.tensor([host_s / args.steps * 1e3, elapsed_local / args.steps * 1e3], device=device, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        hook_launches = int(getattr(reducer, "last_hook_launches", 0))      # of the last TIMED step: the A/B leg below runs paused,
        relaunches = int(getattr(reducer, "relaunches", 0))                 # and its finish() resets the counters
        reducer.paused = reducer.skip_exchange = True
        nab = max(3, min(args.steps, 10))
        step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(nab):
            step()
        barrier()
        no_comm_ms = (time.perf_counter() - t1) / nab * 1e3
        reducer.paused = reducer.skip_exchange = False
        tt = torch.tensor([no_comm_ms], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dp_info = dict(world=world, backend=dist.get_backend(), rccl_ranks=dist.get_world_size(), overlap=bool(reducer.overlap),
                       buckets=len(reducer.buckets), hook_launches_last_step=hook_launches,
                       relaunches=relaunches, grad_mbytes=round(sum(p.numel() for p in params) * 4 / 1e6, 1),
                       rank_ms_per_step_min_max=[round(min(float(a[1]) for a in allr), 3), round(max(float(a[1]) for a in allr), 3)],
                       rank_host_ms_min_max=[round(min(float(a[0]) for a in allr), 2), round(max(float(a[0]) for a in allr), 2)],
                       ms_per_step_without_exchange=round(tt.item(), 3), allreduce_exposed_ms=round(ms_per_step - tt.item(), 3),
                       hw_queues_env=os.environ.get("GPU_MAX_HW_QUEUES"))
        barrier()

    if rank == 0:
        _l = default_lib()
        if _l.test_tune("skip", -1) > 0 or _l.test_tune("noatomic", -1) > 0:
            raise SystemExit("bench.py: a what-if switch (dgsct_test_tune skip / noatomic) is set in this process: the step computed garbage, no line")
        cpu = None
        if world == 1 and args.full and not args.no_cpu_baseline:
            cpu = cpu_baseline(args.backbone)
        line = dict(
            metric="adapter_fwd_bwd_clips_per_sec", value=round(clips_per_s, 2), unit="clips/s", n_gpus=world,
            steps=args.steps, warmup=args.warmup, ms_per_step=round(ms_per_step, 3), higher_is_better=True, scaling=args.scaling,
            vs_baseline=None, dtype=("bf16_fp8" if fp8 else "bf16") if dtype == torch.bfloat16 else "f32", data="synthetic",
            config=dict(workload=f"AVE fine-tune adapter stack (BASELINE configs[1]): {args.backbone} + HTS-AT token/width "
                                 f"shapes, 48 DG-SCT adapters, B={per_gpu_batch} clips/GPU x T=10, r=8 g=2 tk={args.num_tokens} BN+LN on" +
                                 (" (NOT the graded workload: num_tokens > 32 / DGSCT_WIDE_ATTN -- the unfused latent-token attentions of csrc/attn_wide.cpp)"
                                  if args.num_tokens > 32 or os.environ.get("DGSCT_WIDE_ATTN", "0") not in ("", "0") else "") +
                                 (" + HARNESS B: the 12 frozen Swin-V2 blocks / HTS-AT blocks beside the adapter positions in the loop (not the graded workload)"
                                  if args.blocks else ""),
                        global_batch=per_gpu_batch * world, frames_per_clip=T, parallelism=f"dp{world}",
                        step="fwd+bwd" + ("+allreduce" if dp else "") + ("" if args.no_optim else "+adam"),
                        streams=1 if args.serial else 2, hip_graph=use_graph, host_enqueue_ms_per_step=round(host_s / args.steps * 1e3, 2),
                        host_ms_fwdbwd_allreduce_optim=host_ms,
                        host_floor_ms_per_step=host_floor,
                        **({"gpu_ms_fwd_bwd": [round(sum(a.elapsed_time(b) for a, b, _ in phase_ev[-args.steps:]) / args.steps, 2),
                                               round(sum(b.elapsed_time(c) for _, b, c in phase_ev[-args.steps:]) / args.steps, 2)]}
                           if args.phases and len(phase_ev) >= args.steps else {})),
            roofline=roofline, cpu_baseline=cpu, **({"dp": dp_info} if dp_info else {}))
        # RCCL writes its version banner through C stdio: on a pipe it would be flushed at exit, i.e. AFTER this line; drain it
        # first so that the JSON line is the last thing rank 0 prints
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(line), flush=True)
    if dp:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
