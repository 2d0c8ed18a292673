"""GPU parity at the shapes of the BASELINE configs that round 1 never exercised:

* Swin-V2-L widths -- what the reference code actually builds (`swinv2_large_window12_192_22k`, net_trans.py:693):
  C = 192 / 384 / 768 / 1536 (1536 is the upper bound of Plan::validate) -- all four stages, both directions;
* configs[3] AVS-S4: bicubic token remap 64x64 <-> 48x48 and 32x32 <-> 24x24 grids, T = 5, gate before ln_post, no ln_before
  (avs_s4/model/PVT_AVSModel.py:190-197, 239, 272, 308-313);
* configs[4] AVQA: tk = 2, g = 4, no BatchNorm, audio adapters without the output gate (AVQA/net_grd_avst/base_options.py:67-87);
* configs[2] AVVP at its per-GPU batch (B = 32 over DP = 4 -> BT = 80);
* one oracle comparison at the benchmark's BT = 160 (fp32 and bf16) so that the full-size property tests do not hang on
  an unpinned link (fp32@160 frames).

All through the C ABI, against the CPU oracle on identical (bf16-representable for the bf16 runs) inputs."""
import json
import os

import pytest
import torch

from helpers import fp32_err, grad_close_fp32, nrm_err, param_table, rel_err, spec_of
from dgsct_amd import ops
from dgsct_amd._lib import PARAM_NAMES, default_lib
from oracle import dgsct_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_F32 = 1e-3


def _l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def run_case(N, C, No, Co, BT, dtype, flavour="ave", seed=0, over=None):
    kw = {**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS[flavour], **(over or {})}
    cfg = O.AdapterConfig(**kw)
    p = O.random_params(cfg, flavour, seed=seed, scale=0.577)
    if cfg.remap == "bicubic":
        p["_bicubic"] = O.bicubic_matrix(No, N)
    gen = torch.Generator().manual_seed(seed + 1)
    X = torch.randn(BT, N, C, generator=gen)
    Y = torch.randn(BT, No, Co, generator=gen)
    dOut = torch.randn(BT, N, C, generator=gen)
    dMap = torch.randn(BT, N, generator=gen)
    dTmap = torch.randn(BT, generator=gen) if cfg.temporal else None          # cotangent of the per-frame temporal gate
    if dtype == torch.bfloat16:
        X, Y, dOut = X.bfloat16().float(), Y.bfloat16().float(), dOut.bfloat16().float()
    po = {k: v.clone() for k, v in p.items()}
    out_o, map_o, _, s = O.forward(po, X, Y, cfg, training=True)
    spec = spec_of(cfg)
    params = param_table(p, spec, DEV)
    lib = default_lib()
    Xd, Yd = X.to(DEV, dtype).contiguous(), Y.to(DEV, dtype).contiguous()
    prep = ops.prepare(lib, spec, params, dtype, DEV)
    out, amap, _, saved, d = ops.raw_forward(lib, spec, params, prep, Xd, Yd, True)
    masks = None
    if dtype == torch.float32:          # fp32: the oracle differentiates the ReLU branches the device took (see test_adapter_gpu._real_case)
        from helpers import device_relu_masks
        torch.cuda.synchronize()
        masks = device_relu_masks(lib, d, saved, spec, BT, dtype)
    dX_o, dY_o, g_o = O.backward(po, s, cfg, dOut, dMap, dTmap, training=True, masks=masks)
    dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, Xd, Yd, saved, dOut.to(DEV, dtype).contiguous(),
                                     dMap.to(DEV), dTmap.to(DEV) if dTmap is not None else None)
    torch.cuda.synchronize()
    return dict(out=(out, out_o), map=(amap, map_o), dX=(dX, dX_o), dY=(dY, dY_o),
                grads={PARAM_NAMES[i]: (g, g_o[PARAM_NAMES[i]]) for i, g in enumerate(grads)
                       if g is not None and PARAM_NAMES[i] in g_o},
                extra=[PARAM_NAMES[i] for i, g in enumerate(grads) if g is not None and PARAM_NAMES[i] not in g_o],
                missing=[k for k in g_o if k in PARAM_NAMES and grads[PARAM_NAMES.index(k)] is None])


def check_fp32(r):
    bad = [(k, fp32_err(*r[k])) for k in ("out", "map", "dX", "dY") if not fp32_err(*r[k]) < TOL_F32]
    assert not r["extra"] and not r["missing"], (r["extra"], r["missing"])
    assert r["grads"]
    bad += [(k, fp32_err(g, go)) for k, (g, go) in r["grads"].items() if not grad_close_fp32(g, go, TOL_F32, name=k)]
    assert not bad, bad


_B = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_bounds.json")))
_EMU = [v for k, v in _B.items() if k.startswith(("real_", "cfg_"))]
CAP_DX = max(v["dX"] for v in _EMU)             # largest emulator-derived bound among the emulated real-shape cases
CAP_DY = max(v["dY"] for v in _EMU)
CAP_W = max(max(v["grads"].values()) for v in _EMU)


def check_bf16(r, key=None):
    """outputs: BASELINE's 1e-2 in relative L2 (worst element within 4e-2 of max|ref|: the gate-before-LayerNorm flavours put
    a few elements at 3 %).  Gradients: the emulator-derived relative-L2 bound of the case (tests/golden/bf16_bounds.json,
    key "cfg_*": the stage-2/3 shapes, whose host emulation takes seconds) or, for the stage-0/1 shapes (minutes per
    emulation), the largest bound among the emulated cases -- see tests/test_adapter_gpu.py's docstring for why a bf16
    gradient has no 1e-2 bound against fp32 under ANY rounding."""
    for k in ("out", "map"):
        assert torch.isfinite(r[k][0].float()).all(), k
        assert _l2(*r[k]) < 1e-2, (k, _l2(*r[k]))
        assert nrm_err(*r[k]) < 4e-2, (k, nrm_err(*r[k]))
    b = _B.get(key) if key else None
    assert _l2(*r["dX"]) < (b["dX"] if b else CAP_DX), ("dX", _l2(*r["dX"]))
    assert _l2(*r["dY"]) < (b["dY"] if b else CAP_DY), ("dY", _l2(*r["dY"]))
    for k, (g, go) in r["grads"].items():
        assert torch.isfinite(g).all(), k
        if b and k in b["grads"]:
            assert _l2(g, go.reshape(-1)) < b["grads"][k], (k, _l2(g, go.reshape(-1)), b["grads"][k])
        elif go.dim() >= 2 and go.numel() > go.shape[0] and k != "ln_before.bias":
            assert _l2(g, go.reshape(-1)) < CAP_W, (k, _l2(g, go.reshape(-1)))


def _key(flavour, shape):
    k = f"cfg_{flavour}_{shape[0]}x{shape[1]}"
    return k if k in _B else None


# (N, C, No, Co): Swin-V2-L visual widths 192/384/768/1536 against HTS-AT 96/192/384/768, visual and audio direction
SWIN_L = [(2304, 192, 4096, 96), (4096, 96, 2304, 192), (576, 384, 1024, 192), (1024, 192, 576, 384),
          (144, 768, 256, 384), (256, 384, 144, 768), (36, 1536, 64, 768), (64, 768, 36, 1536)]


@pytest.mark.parametrize("shape", SWIN_L)
def test_swin_large_widths_fp32(shape):
    check_fp32(run_case(*shape, BT=10, dtype=torch.float32))


@pytest.mark.parametrize("shape", SWIN_L)
def test_swin_large_widths_bf16(shape):
    check_bf16(run_case(*shape, BT=10, dtype=torch.bfloat16), _key("ave", shape))


# configs[3] AVS-S4 (T = 5 frames per clip): the bicubic resize is a dense [N, No] operator between square token grids
AVS = [(2304, 192, 4096, 96), (4096, 96, 2304, 192), (576, 384, 1024, 192), (1024, 192, 576, 384), (36, 1536, 64, 768)]


@pytest.mark.parametrize("shape", AVS)
def test_avs_s4_swin_large_fp32(shape):
    check_fp32(run_case(*shape, BT=5, dtype=torch.float32, flavour="avs_s4"))


@pytest.mark.parametrize("shape", [AVS[0], AVS[3], AVS[4]])
def test_avs_s4_swin_large_bf16(shape):
    check_bf16(run_case(*shape, BT=10, dtype=torch.bfloat16, flavour="avs_s4"), _key("avs_s4", shape))


# configs[4] AVQA: tk = 2, g = 4, no BN; the audio adapters are built with use_gate = 0 (AVQA/train.sh)
@pytest.mark.parametrize("shape,use_gate", [((2304, 192, 4096, 96), True), ((4096, 96, 2304, 192), False),
                                            ((144, 768, 256, 384), True), ((256, 384, 144, 768), False),
                                            ((36, 1536, 64, 768), True), ((64, 768, 36, 1536), False)])
def test_avqa_swin_large_fp32(shape, use_gate):
    check_fp32(run_case(*shape, BT=10, dtype=torch.float32, flavour="avqa", over=dict(use_gate=use_gate)))


@pytest.mark.parametrize("shape,use_gate", [((2304, 192, 4096, 96), True), ((256, 384, 144, 768), False),
                                            ((36, 1536, 64, 768), True)])
def test_avqa_swin_large_bf16(shape, use_gate):
    check_bf16(run_case(*shape, BT=10, dtype=torch.bfloat16, flavour="avqa", over=dict(use_gate=use_gate)), _key("avqa", shape))


# the two flavours no BASELINE config names, at real shapes (the goldens hold them at toy sizes only): AVS-MS3 (conv remap,
# alpha 0.2 / beta 0.1, gate before ln_post, T = 5) and pretrain / few-shot / zero-shot (temporal gate, gamma, 3-tuple output)
@pytest.mark.parametrize("shape", [(576, 384, 1024, 192), (36, 1536, 64, 768)])
def test_avs_ms3_fp32(shape):
    check_fp32(run_case(*shape, BT=5, dtype=torch.float32, flavour="avs_ms3"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(144, 512, 256, 384), (64, 768, 36, 1024)])
def test_pretrain_temporal_gate(shape, dtype):
    r = run_case(*shape, BT=20, dtype=dtype, flavour="pretrain")
    assert "temporal_gated.0.weight" in r["grads"] and "temporal_gated.0.bias" in r["grads"]
    (check_fp32 if dtype == torch.float32 else check_bf16)(r)


# configs[2] AVVP: B = 32 clips over DP = 4 -> 80 frames per GPU
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_avvp_per_gpu_batch(dtype):
    r = run_case(144, 512, 256, 384, BT=80, dtype=dtype, flavour="avvp")
    (check_fp32 if dtype == torch.float32 else check_bf16)(r)


# the benchmark's BT = 160 against the oracle (stage-2 and stage-3 shapes of BASELINE configs[1]: seconds on the CPU)
@pytest.mark.parametrize("shape", [(144, 512, 256, 384), (64, 768, 36, 1024)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_batch_against_oracle(shape, dtype):
    r = run_case(*shape, BT=160, dtype=dtype)
    (check_fp32 if dtype == torch.float32 else check_bf16)(r)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,flavour", [((4096, 96, 2304, 128), "ave"), ((576, 256, 1024, 192), "ave"), ((1024, 192, 576, 256), "avs_s4")])
def test_fused_row_pass_equals_the_three_launches(shape, flavour, dtype):
    """modln_gproj (modulation + ln_before + down-projection + BN1 sums, one kernel at stages 0-1) against the separate
    modln_fwd / gproj_narrow / bn_stats launches it replaces (dgsct_test_tune "rowfuse"): same rounding points, so the
    stored tensors agree to the last bit or two of fp32 summation order, and everything downstream with them."""
    N, C, No, Co = shape
    BT = 10
    kw = {**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS[flavour]}
    cfg = O.AdapterConfig(**kw)
    p = O.random_params(cfg, flavour, seed=3, scale=0.577)
    if cfg.remap == "bicubic":
        p["_bicubic"] = O.bicubic_matrix(No, N)
    spec = spec_of(cfg)
    lib = default_lib()
    gen = torch.Generator().manual_seed(11)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    dMap = torch.randn(BT, N, generator=gen).to(DEV)
    res = []
    old = lib.test_tune("rowfuse", -1)
    try:
        for mode in (1, 0):
            lib.test_tune("rowfuse", mode)
            params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)       # (BN running stats are updated in place)
            prep = ops.prepare(lib, spec, params, dtype, DEV)
            out, amap, _, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, dMap, None)
            torch.cuda.synchronize()
            bn = [params[PARAM_NAMES.index(n)].clone() for n in ("bn1.running_mean", "bn1.running_var")]
            res.append((out.float(), amap, dX.float(), dY.float(), [g.clone() if g is not None else None for g in grads], bn))
    finally:
        lib.test_tune("rowfuse", old)
    tol = 2e-5 if dtype == torch.float32 else 1e-2      # bf16: a 1-ulp difference of a stored BN statistic can flip roundings downstream
    a, b = res
    for i, name in enumerate(("out", "map", "dX", "dY")):
        assert _l2(a[i], b[i]) < tol, (name, _l2(a[i], b[i]))
    for n, (ra, rb) in zip(("bn1.running_mean", "bn1.running_var"), zip(a[5], b[5])):
        assert _l2(ra, rb) < 1e-5, (n, _l2(ra, rb))
    for name, ga, gb in zip(PARAM_NAMES, a[4], b[4]):
        if ga is None or ga.float().norm() == 0 or name in ("ln_before.bias", "fc_affine_v_s_att.bias", "fc.bias"):
            continue        # (those three are cancellation residues: a bias in front of a normalisation / softmax, helpers.FP32_RESIDUES)
        assert _l2(ga, gb) < (1e-4 if dtype == torch.float32 else 2e-2), (name, _l2(ga, gb))


@pytest.mark.parametrize("shape,flavour,BT", [((4096, 96, 2304, 128), "ave", 10), ((2304, 128, 4096, 96), "ave", 10), ((576, 256, 1024, 192), "ave", 10),
                                              ((1024, 192, 576, 256), "ave", 20), ((1024, 192, 576, 256), "avs_s4", 10), ((2304, 128, 4096, 96), "pretrain", 10),
                                              ((4096, 96, 2304, 128), "avqa", 10)])
def test_fused_gate_passes_equal_the_launches_they_replace(shape, flavour, BT):
    """fused_gate.hip (bf16, C <= 256: spatial gate + modulation + ln_before + down-projection + BN1 sums in one pass over X1, and its
    backward counterpart) against the unfused launches (dgsct_test_tune "gatefuse" = 0) on the same inputs: the two differ in where
    bf16 roundings fall (the frame's channel gate is folded into the weights instead of into Xc), so stored tensors agree to bf16
    rounding and everything downstream to the run-to-run spread of a bf16 evaluation."""
    N, C, No, Co = shape
    kw = {**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS[flavour]}
    cfg = O.AdapterConfig(**kw)
    p = O.random_params(cfg, flavour, seed=3, scale=0.577)
    if cfg.remap == "bicubic":
        p["_bicubic"] = O.bicubic_matrix(No, N)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(11)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    dMap = torch.randn(BT, N, generator=gen).to(DEV)
    res = []
    old = lib.test_tune("gatefuse", -1)
    assert old == 1
    try:
        for mode in (1, 0):
            lib.test_tune("gatefuse", mode)
            params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
            prep = ops.prepare(lib, spec, params, dtype, DEV)
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
            torch.cuda.synchronize()
            regs = lib.saved_regions(d)
            keep = {}
            for name, (n, dt) in {"sl": (BT * N, torch.float32), "X3": (BT * N * C, dtype), "Zp": (BT * N * (C // cfg.r), dtype),
                                  "mu_b": (BT * N, torch.float32), "rstd_b": (BT * N, torch.float32)}.items():
                off, nb = regs[name]
                keep[name] = saved[off:off + n * (4 if dt == torch.float32 else 2)].view(dt).float().clone()
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, dMap, None)
            torch.cuda.synchronize()
            bn = [params[PARAM_NAMES.index(n)].clone() for n in ("bn1.running_mean", "bn1.running_var")] if cfg.use_bn else []
            res.append((out.float(), amap, dX.float(), dY.float(), [g.clone() if g is not None else None for g in grads], bn, keep))
    finally:
        lib.test_tune("gatefuse", old)
    a, b = res
    for name in ("sl", "mu_b", "rstd_b"):
        if cfg.ln_before or name == "sl":
            assert _l2(a[6][name], b[6][name]) < 1e-2, (name, _l2(a[6][name], b[6][name]))
    assert _l2(a[6]["X3"], b[6]["X3"]) < 1e-2 and _l2(a[6]["Zp"], b[6]["Zp"]) < 1.5e-2, (_l2(a[6]["X3"], b[6]["X3"]), _l2(a[6]["Zp"], b[6]["Zp"]))
    for i, name in enumerate(("out", "map")):
        assert _l2(a[i], b[i]) < 1e-2, (name, _l2(a[i], b[i]))
    for i, name in ((2, "dX"), (3, "dY")):
        assert _l2(a[i], b[i]) < 6e-2, (name, _l2(a[i], b[i]))           # un-pinned ReLU masks: two bf16 evaluations differ by 3-5 %
    if a[5]:        # BatchNorm-1 running statistics (the fused pass sums with its own shift): means relative to the channel's spread
        sd = b[5][1].sqrt()
        assert float(((a[5][0] - b[5][0]).abs() / sd).max()) < 2e-3 and _l2(a[5][1], b[5][1]) < 5e-3


@pytest.mark.parametrize("shape,dtype,training", [((144, 512, 256, 384), torch.bfloat16, True), ((64, 768, 36, 1024), torch.bfloat16, True),
                                                  ((576, 256, 1024, 192), torch.bfloat16, True), ((144, 512, 256, 384), torch.float32, True),
                                                  ((256, 384, 144, 512), torch.bfloat16, False)])
def test_bn_finalise_folded_into_its_consumer(shape, dtype, training):
    """BatchNorm's finalisation (mean / rstd / scale / shift from the batch sums, running statistics) runs inside the pass that
    applies it -- affine_act_bn for BN1, tail_fwd for BN2 -- instead of as two one-workgroup launches on the dependency chain.
    Against the unfolded schedule (dgsct_test_tune "bnfold" = 0) on the same inputs: same arithmetic per channel, so outputs,
    saved BN vectors and running statistics must agree to the last bit or two (fp32: rsqrt / fma contraction differences only)."""
    N, C, No, Co = shape
    BT = 10
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS["ave"]})
    p = O.random_params(cfg, "ave", seed=5, scale=0.577)
    spec = spec_of(cfg)
    lib = default_lib()
    gen = torch.Generator().manual_seed(13)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    res = []
    old = lib.test_tune("bnfold", -1)
    assert old == 1
    try:
        for mode in (1, 0):
            lib.test_tune("bnfold", mode)
            params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
            prep = ops.prepare(lib, spec, params, dtype, DEV)
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, training)
            torch.cuda.synchronize()
            regs = lib.saved_regions(d)
            keep = {}
            for name, n in (("bn1", 4 * (C // cfg.r)), ("bn2", 4 * C)):
                off, nb = regs[name]
                keep[name] = saved[off:off + 4 * n].view(torch.float32).clone()
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, None, None)
            torch.cuda.synchronize()
            run = [params[PARAM_NAMES.index(n)].clone() for n in ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")]
            res.append((out.float(), dX.float(), dY.float(), keep, run))
    finally:
        lib.test_tune("bnfold", old)
    a, b = res
    for name in ("bn1", "bn2"):      # (the batch sums themselves come from fp32 atomics: two runs differ in the last bits)
        assert _l2(a[3][name], b[3][name]) < 2e-5, (name, _l2(a[3][name], b[3][name]))
    for ra, rb in zip(a[4], b[4]):
        assert _l2(ra, rb) < 2e-5
    tol = 1e-6 if dtype == torch.float32 else 4e-3      # bf16: a last-bit difference of a scale moves a few outputs by one bf16 ulp
    assert _l2(a[0], b[0]) < tol, ("out", _l2(a[0], b[0]))
    # backward: two RUNS of one schedule already differ (fp32 atomic sums feed ReLU decisions near zero): 1e-3-class in fp32 as well
    for i, name in ((1, "dX"), (2, "dY")):
        assert _l2(a[i], b[i]) < (2e-3 if dtype == torch.float32 else 4e-2), (name, _l2(a[i], b[i]))


@pytest.mark.parametrize("shape,flavour", [((144, 512, 256, 384), "ave"), ((256, 384, 144, 512), "ave"), ((36, 1024, 64, 768), "ave"),
                                           ((576, 256, 1024, 192), "pretrain"), ((2304, 128, 4096, 96), "avqa")])
def test_folded_gate_products_equal_the_launches_they_replace(shape, flavour):
    """gemm_skinny_fused_k (the operand transforms m1 = aq1 * mean_N vq1 and dpre = dch ch (1 - ch), dm1's two consumers and both `da`
    products folded into the skinny gate-MLP products) against the separate elementwise + product launches (dgsct_test_tune
    "skfuse" = 0) on the same inputs, bf16: every rounding point is the same (operands rounded to bf16 once, fp32 accumulation), so
    only the summation order inside a product differs."""
    N, C, No, Co = shape
    BT = 10
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS[flavour]})
    p = O.random_params(cfg, flavour, seed=7, scale=0.577)
    if cfg.remap == "bicubic":
        p["_bicubic"] = O.bicubic_matrix(No, N)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(17)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    dMap = torch.randn(BT, N, generator=gen).to(DEV)
    res = []
    old = lib.test_tune("skfuse", -1)
    assert old == 1
    try:
        for mode in (1, 0):
            lib.test_tune("skfuse", mode)
            params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
            prep = ops.prepare(lib, spec, params, dtype, DEV)
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
            torch.cuda.synchronize()
            regs = lib.saved_regions(d)
            keep = {}
            for name, (n, dt) in {"m1": (BT * C, dtype), "q": (BT * (C // 2), dtype), "ch": (BT * C, torch.float32)}.items():
                off, nb = regs[name]
                keep[name] = saved[off:off + n * (4 if dt == torch.float32 else 2)].view(dt).float().clone()
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, dMap, None)
            torch.cuda.synchronize()
            res.append((out.float(), amap, dX.float(), dY.float(), [g.clone() if g is not None else None for g in grads], keep))
    finally:
        lib.test_tune("skfuse", old)
    a, b = res
    assert torch.equal(a[5]["m1"], b[5]["m1"])                      # same product, same single rounding
    assert _l2(a[5]["q"], b[5]["q"]) < 4e-3 and _l2(a[5]["ch"], b[5]["ch"]) < 1e-3
    for i, name in enumerate(("out", "map")):
        assert _l2(a[i], b[i]) < 1e-2, (name, _l2(a[i], b[i]))
    for i, name in ((2, "dX"), (3, "dY")):
        assert _l2(a[i], b[i]) < 6e-2, (name, _l2(a[i], b[i]))       # un-pinned ReLU masks downstream of q
    for name, ga, gb in zip(PARAM_NAMES, a[4], b[4]):
        if ga is None or ga.float().norm() == 0 or name in ("ln_before.bias", "fc_affine_v_s_att.bias", "fc.bias"):
            continue
        assert _l2(ga, gb) < 8e-2, (name, _l2(ga, gb))


@pytest.mark.parametrize("shape,flavour,BT", [((4096, 96, 2304, 128), "ave", 10), ((2304, 128, 4096, 96), "ave", 10), ((2304, 128, 4096, 96), "pretrain", 10),
                                              ((4096, 96, 2304, 128), "avqa", 20), ((1024, 96, 576, 128), "ave", 7)])
def test_vq1_without_the_tensor_equals_the_launches_it_replaces(shape, flavour, BT):
    """vq1_fwd_k / vq1_bwd_k (stage 0, bf16: mean_N relu(X1 Wv1^T + b) in one pass over X1 with nothing stored; the backward recomputes
    the ReLU decisions and applies dX1 += dvq1 Wv1 in place) against product + column sum / ReLU backward + product (dgsct_test_tune
    "vq1fuse" = 0) on the same inputs.  Forward: the fused pass sums fp32 values, the unfused one bf16-rounded ones (mvq1 agrees to
    ~1e-3).  Backward: same ReLU decisions (same product bits) and the same single rounding of dvq1 and of dX1."""
    N, C, No, Co = shape
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS[flavour]})
    p = O.random_params(cfg, flavour, seed=9, scale=0.577)
    if cfg.remap == "bicubic":
        p["_bicubic"] = O.bicubic_matrix(No, N)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(19)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    dMap = torch.randn(BT, N, generator=gen).to(DEV)
    res = []
    old = lib.test_tune("vq1fuse", -1)
    assert old == 1
    try:
        for mode in (1, 0):
            lib.test_tune("vq1fuse", mode)
            params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
            prep = ops.prepare(lib, spec, params, dtype, DEV)
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
            torch.cuda.synchronize()
            regs = lib.saved_regions(d)
            off, nb = regs["mvq1"]
            mvq1 = saved[off:off + 4 * BT * C].view(torch.float32).clone()
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, dMap, None)
            torch.cuda.synchronize()
            res.append((out.float(), amap, dX.float(), dY.float(), [g.clone() if g is not None else None for g in grads], mvq1))
    finally:
        lib.test_tune("vq1fuse", old)
    a, b = res
    assert _l2(a[5], b[5]) < 2e-3, _l2(a[5], b[5])
    for i, name in enumerate(("out", "map")):
        assert _l2(a[i], b[i]) < 1e-2, (name, _l2(a[i], b[i]))
    for i, name in ((2, "dX"), (3, "dY")):
        assert _l2(a[i], b[i]) < 6e-2, (name, _l2(a[i], b[i]))       # un-pinned ReLU masks downstream of the gate
    for name, ga, gb in zip(PARAM_NAMES, a[4], b[4]):
        if ga is None or ga.float().norm() == 0 or name in ("ln_before.bias", "fc_affine_v_s_att.bias", "fc.bias"):
            continue
        assert _l2(ga, gb) < 8e-2, (name, _l2(ga, gb))


@pytest.mark.parametrize("shape,dtype", [((4096, 96, 2304, 128), torch.bfloat16), ((1024, 192, 576, 256), torch.bfloat16), ((576, 256, 1024, 192), torch.bfloat16),
                                         ((1024, 96, 576, 128), torch.float32)])
def test_bn2_backward_inside_the_narrow_projection(shape, dtype):
    """gproj_narrow_k<BNB>: BatchNorm-2's backward applied to the cotangent row on its way into the grouped up-projection's backward
    (one pass, dOp stored from it) against bn_bwd_apply + gproj_narrow (dgsct_test_tune "rowfuse" = 0).  The projection multiplies the
    value as stored: per element the two schedules do the same arithmetic."""
    N, C, No, Co = shape
    BT = 6
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS["ave"]})
    p = O.random_params(cfg, "ave", seed=11, scale=0.577)
    spec = spec_of(cfg)
    lib = default_lib()
    gen = torch.Generator().manual_seed(29)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
    prep = ops.prepare(lib, spec, params, dtype, DEV)
    res = []
    old = lib.test_tune("rowfuse", -1)
    try:
        for mode in (1, 0):
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, False)     # eval mode: nothing in the parameters moves between the two runs
            lib.test_tune("rowfuse", mode)
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, None, None)
            torch.cuda.synchronize()
            lib.test_tune("rowfuse", old)
            res.append((dX.clone(), dY.clone(), [g.clone() if g is not None else None for g in grads]))
    finally:
        lib.test_tune("rowfuse", old)
    a, b = res
    # identical arithmetic per element; the reductions around it (BN sums, per-frame gate gradients) are fp32 atomics whose order
    # differs from run to run, so "the same" means to a few ulps of the stored type, not torch.equal
    tol = 1e-5 if dtype == torch.float32 else 3e-3
    assert _l2(a[0].float(), b[0].float()) < tol and _l2(a[1].float(), b[1].float()) < tol, (_l2(a[0].float(), b[0].float()), _l2(a[1].float(), b[1].float()))
    for name, ga, gb in zip(PARAM_NAMES, a[2], b[2]):
        if ga is not None and name in ("up_sampler.weight", "down_sampler.weight", "bn1.bias", "bn1.weight", "bn2.bias", "bn2.weight"):
            assert _l2(ga, gb) < tol, (name, _l2(ga, gb))


@pytest.mark.parametrize("shape", [(4096, 96, 2304, 128), (2304, 128, 4096, 96)])
def test_weight_gradients_on_gemm_tall_equal_the_tiled_engine(shape):
    """the five weight gradients over the token rows (dWu, dWd with their group slabs starting on column 6 at C = 96; dWv2, dWv1, dWc) on
    gemm_tall.hip ("gemmtall" = 2: from 16 384 rows, so that 10 frames reach it) against the tiled engine's split-K products
    ("gemmtall" = 0) inside one adapter backward: same operands, fp32 accumulation in a different order"""
    N, C, No, Co = shape
    BT = 10
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS["ave"]})
    p = O.random_params(cfg, "ave", seed=17, scale=0.577)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(37)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
    prep = ops.prepare(lib, spec, params, dtype, DEV)
    res = []
    old = lib.test_tune("gemmtall", -1)
    try:
        for mode in (2, 0):
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, False)     # eval mode: the parameters do not move
            lib.test_tune("gemmtall", mode)
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved, dOut, None, None)
            torch.cuda.synchronize()
            lib.test_tune("gemmtall", old)
            res.append({n: g.clone() for n, g in zip(PARAM_NAMES, grads) if g is not None})
    finally:
        lib.test_tune("gemmtall", old)
    a, b = res
    for name in ("up_sampler.weight", "down_sampler.weight", "fc_affine_video_1.weight", "fc_affine_video_2.weight", "fc.weight", "conv_adapter.weight"):
        if name in a:
            assert _l2(a[name], b[name]) < 2e-3, (name, _l2(a[name], b[name]))


@pytest.mark.parametrize("shape,BT,masks", [((576, 256, 1024, 192), 10, (0, 15)), ((1024, 192, 576, 256), 10, (0, 15)),
                                            ((144, 512, 256, 384), 20, (0, 15, 31)), ((256, 384, 144, 512), 20, (0, 15, 31)),
                                            ((36, 1024, 64, 768), 20, (0, 15, 31)), ((64, 768, 36, 1024), 10, (0, 15, 4 + 32)),
                                            ((144, 512, 256, 384), 160, (0, 15))])
def test_fused_gemm_hooks_equal_the_launches_they_replace(shape, BT, masks):
    """round 5, csrc/gemm_fx.hip: the backward products of the late-stage schedule with the elementwise launch in front of them folded
    into the staging of their A operand (ReLU backward of vq2 / vq1: relu_bwd_scale; BatchNorm backward of dO / dZ: bn_bwd_apply) and
    the channel-gate backward (xc_bwd) into the epilogue, against the separate launches (dgsct_test_tune "gemmfx" = 0) on the same
    inputs.  Same operands and the same rounding points (the transformed operand and E(dXc) are rounded to bf16 exactly where the
    separate launches stored them); what differs is the fp32 summation order of the per-frame / per-channel sums and the form of the two
    query-layer bias gradients (counts x value instead of a column sum of the rounded tensor)."""
    N, C, No, Co = shape
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS["ave"]})
    p = O.random_params(cfg, "ave", seed=11, scale=0.577)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(29)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    dMap = torch.randn(BT, N, generator=gen).to(DEV)
    res = {}
    old = lib.test_tune("gemmfx", -1)
    assert old == 15 + 64 + 128                # (64 / 128: the forward sites, exercised by the test below)
    # ONE forward (it does not depend on the switch; two forwards differ in the last bits of their atomically summed batch statistics),
    # every backward on its own copy of the saved activations (the separate launches overwrite vq1 / vq2 in place)
    params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
    prep = ops.prepare(lib, spec, params, dtype, DEV)
    out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
    torch.cuda.synchronize()
    try:
        for mode in masks:
            lib.test_tune("gemmfx", mode)
            dX, dY, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved.clone(), dOut, dMap, None)
            torch.cuda.synchronize()
            res[mode] = (dX.float(), dY.float(), [g.clone() if g is not None else None for g in grads])
    finally:
        lib.test_tune("gemmfx", old)
    ref = res[0]
    for mode in masks[1:]:
        a = res[mode]
        for i, name in ((0, "dX"), (1, "dY")):
            assert _l2(a[i], ref[i]) < 4e-3, (mode, name, _l2(a[i], ref[i]))
        for name, ga, gb in zip(PARAM_NAMES, a[2], ref[2]):
            if ga is None or gb.float().norm() == 0 or name in ("ln_before.bias", "fc_affine_v_s_att.bias", "fc.bias", "gate", "gate_av"):
                continue
            assert _l2(ga, gb) < 8e-3, (mode, name, _l2(ga, gb))


@pytest.mark.parametrize("shape,BT", [((576, 256, 1024, 192), 10), ((144, 512, 256, 384), 20), ((256, 384, 144, 512), 20), ((36, 1024, 64, 768), 20),
                                      ((64, 768, 36, 1024), 10), ((144, 512, 256, 384), 160)])
def test_forward_gemm_epilogues_equal_the_reductions_they_replace(shape, BT):
    """round 5, csrc/gemm_fx.hip forward sites: vq1 = relu(X1 Wv1^T + b) with its per-frame column sums (mean_N vq1) and positive
    counts in the product's epilogue ("gemmfx" bit 64: no colsum pass), and the two bottleneck products with their BatchNorm sums in
    the epilogue (bit 128: no bn_stats passes; sums of the values as stored, shift 0 instead of row 0) -- against the separate
    reductions on the same inputs: the per-frame means, the counts (exact), the BatchNorm statistics and the outputs."""
    N, C, No, Co = shape
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS["ave"]})
    p = O.random_params(cfg, "ave", seed=13, scale=0.577)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(31)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    res = {}
    old = lib.test_tune("gemmfx", -1)
    try:
        for mode in (15, 15 + 64 + 128):
            lib.test_tune("gemmfx", mode)
            params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
            prep = ops.prepare(lib, spec, params, dtype, DEV)
            out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
            torch.cuda.synchronize()
            regs = lib.saved_regions(d)
            grab = lambda nm, n: saved[regs[nm][0]:regs[nm][0] + 4 * n].view(torch.float32).clone()
            ds = C // 8
            res[mode] = dict(out=out.float(), map=amap.clone(), mvq1=grab("mvq1", BT * C), cnt1=grab("cnt1", BT * C), bn1=grab("bn1", 4 * ds),
                             bn2=grab("bn2", 4 * C), rm2=params[PARAM_NAMES.index("bn2.running_mean")].clone(),
                             rv1=params[PARAM_NAMES.index("bn1.running_var")].clone())
    finally:
        lib.test_tune("gemmfx", old)
    a, b = res[15], res[15 + 64 + 128]
    assert torch.equal(a["cnt1"], b["cnt1"])                                       # same product bits, same ReLU decisions: exact counts
    assert _l2(b["mvq1"], a["mvq1"]) < 1e-5, _l2(b["mvq1"], a["mvq1"])            # fp32 sums of the same bf16 values, another order
    for k in ("bn1", "bn2", "rm2", "rv1"):
        assert _l2(b[k], a[k]) < 2e-4, (k, _l2(b[k], a[k]))                      # (mean | rstd | scale | shift) from sums with another shift
    assert _l2(b["out"], a["out"]) < 4e-3 and _l2(b["map"], a["map"]) < 1e-3, (_l2(b["out"], a["out"]), _l2(b["map"], a["map"]))


@pytest.mark.parametrize("shape,BT", [((2304, 128, 4096, 96), 4), ((4096, 96, 2304, 128), 3), ((576, 256, 1024, 192), 10), ((144, 512, 256, 384), 160),
                                      ((36, 1024, 64, 768), 20), ((64, 768, 36, 1536), 7)])
def test_grouped_frame_deep_weight_gradients_equal_the_four_launches(shape, BT):
    """round 5, csrc/gemm_wgbt.hip: d fc_affine_v_c_att / _bottleneck / _audio_1 / _audio_2 .weight -- the four weight gradients that contract
    over the frames only -- as one launch of 64 x 64 tiles against the four tiled-engine launches ("wgbt" = 0) on the same saved activations:
    same bf16 operands, fp32 accumulation either way -> equal to summation order; widths that are not multiples of 64 (C / 2 = 48), frame
    counts that are not multiples of 16 or 64 (3, 7, 20, 160)."""
    N, C, No, Co = shape
    cfg = O.AdapterConfig(**{**dict(N=N, C=C, No=No, Co=Co, tk=32, r=8, g=2), **O.FLAVOURS["ave"]})
    p = O.random_params(cfg, "ave", seed=5, scale=0.577)
    spec = spec_of(cfg)
    lib = default_lib()
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(31)
    X = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    Y = torch.randn(BT, No, Co, generator=gen).to(DEV, dtype).contiguous()
    dOut = torch.randn(BT, N, C, generator=gen).to(DEV, dtype).contiguous()
    dMap = torch.randn(BT, N, generator=gen).to(DEV)
    params = param_table({k: v.clone() for k, v in p.items()}, spec, DEV)
    prep = ops.prepare(lib, spec, params, dtype, DEV)
    out, amap, tmap, saved, d = ops.raw_forward(lib, spec, params, prep, X, Y, True)
    torch.cuda.synchronize()
    res = {}
    old = lib.test_tune("wgbt", -1)
    assert old == 1
    try:
        for mode in (0, 1):
            lib.test_tune("wgbt", mode)
            _, _, grads = ops.raw_backward(lib, spec, d, params, prep, X, Y, saved.clone(), dOut, dMap, None)
            torch.cuda.synchronize()
            res[mode] = {n: g.clone() for n, g in zip(PARAM_NAMES, grads) if g is not None}
    finally:
        lib.test_tune("wgbt", old)
    names = ("fc_affine_v_c_att.weight", "fc_affine_bottleneck.weight", "fc_affine_audio_1.weight", "fc_affine_audio_2.weight")
    for n in names:
        a, b = res[1][n], res[0][n]
        assert torch.isfinite(a).all() and b.float().norm() > 0
        # (the two backward passes are separate runs: the operands dpa2 / dpre are ROUNDED products of the atomically summed `u` / `dch`, whose
        #  last-bit run-to-run noise moves a few of their bf16 roundings by one ulp (2^-9): ~1e-4 at 160 frames, up to ~1e-3 at 3 frames x 48
        #  channels -- seen once in ~30 runs of the suite at a 1e-3 bound.  A wrong tile or a dropped frame is an O(1) error.)
        assert _l2(a, b) < 4e-3, (n, _l2(a, b))
    for n in res[0]:                                   # ... and nothing else moved (same forward, same chain)
        if n not in names and res[0][n].float().norm() > 0 and n not in ("ln_before.bias", "fc_affine_v_s_att.bias", "fc.bias", "gate", "gate_av"):
            assert _l2(res[1][n], res[0][n]) < 8e-3, (n, _l2(res[1][n], res[0][n]))     # (two runs: atomically summed statistics, as in the test above)
