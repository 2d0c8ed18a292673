"""The trainable front end on the device: ``dgsct_patch_embed_backward_params`` (csrc/frontend.hip) through
``HTSATFrontEnd(trainable=True, fused=True)`` / ``PatchEmbed(trainable=True, fused=True)`` against the differentiable float64
restatement of tests/test_frontend_train_cpu.py.

Bound: ``helpers.fp32_err < 1e-3`` on every gradient, for fp32 AND bf16 tokens (the backward recomputes in fp32 from a dOut that is exact
in either dtype; the fp32 ATen evaluation of the reference itself sits at 2e-7 .. 4e-6).  bf16 tokens: ``helpers.nrm_err < 1e-2``."""
import functools
import os
import sys

import pytest
import torch

import dgsct_amd
from dgsct_amd import HTSATFrontEnd, PatchEmbed, frontend, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R                    # noqa: E402
from helpers import fp32_err, nrm_err       # noqa: E402
from test_frontend_train_cpu import FOUR, SIX, audio_grads64, cotangent, image_grads64, module_grads      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

#        (B, L)            frames   what it exercises
CASES = [(2, 3200),      # T = 11   the smallest stretch source
         (3, 5000),      # T = 16   odd B T, L not a multiple of the hop
         (1, 327360)]    # T = 1024 the no-interpolation path
IDS = ["smallest", "ragged", "no-interp"]


@functools.lru_cache(maxsize=None)
def _wave(B, L):
    """(waveform, float64 log-mel): computed once, shared, never modified"""
    x = R.signal(B, L)
    return x, R.logmel(x)


def _module(embed=96, **kw):
    return R.randomise(HTSATFrontEnd(embed_dim=embed, **kw), 2)


@functools.lru_cache(maxsize=None)
def _reference(B, L, training, embed, dtype):
    """(float64 gradients, float64 tokens, running_mean', running_var') for the cotangent of this dtype"""
    lm = _wave(B, L)[1]
    sd = _module(embed).state_dict()
    grads, tok = audio_grads64(lm, sd, training, cotangent((B, 4096, embed), dtype))
    _, rm, rv = R.audio_tokens(lm, sd, training) if training else (None, None, None)
    return grads, tok, rm, rv


def _check_audio(B, L, training, embed, dtype):
    x = _wave(B, L)[0].to(DEV)
    ref, tok64, rm, rv = _reference(B, L, training, embed, dtype)
    m = _module(embed, out_dtype=dtype, trainable=True, fused=True).to(DEV).train(training)
    tok = m(x)
    assert tok.shape == (B, 4096, embed) and tok.dtype == dtype and tok.requires_grad
    assert "PatchEmbedTrain" in type(tok.grad_fn).__name__
    if dtype == torch.float32:
        assert fp32_err(tok, tok64) < 1e-3
    else:
        assert nrm_err(tok, tok64) < 1e-2
    frozen = _module(embed, out_dtype=dtype).to(DEV).train(training)
    assert torch.equal(tok.detach(), frozen(x))                              # bit for bit the frozen module's tokens
    tok.backward(cotangent((B, 4096, embed), dtype).to(DEV))
    got = module_grads(m)
    for k in SIX:
        assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape, k
        err = fp32_err(got[k], ref[k])
        print(f"[{B}, {L}] training={training} embed={embed} {dtype} {k}: {err:.3e}")
        assert err < 1e-3, k
    assert m.logmel_extractor.melW.grad is None
    if training:
        assert int(m.bn0.num_batches_tracked) == 1
        assert ((m.bn0.running_mean.double().cpu() - rm).abs() / rm.abs().clamp_min(1e-3)).max().item() < 1e-4
        assert ((m.bn0.running_var.double().cpu() - rv).abs() / rv).max().item() < 1e-4
        assert torch.equal(m.bn0.running_mean, frozen.bn0.running_mean) and torch.equal(m.bn0.running_var, frozen.bn0.running_var)
    else:
        assert int(m.bn0.num_batches_tracked) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("B,L", CASES, ids=IDS)
def test_audio_gradients(B, L, training, dtype):
    _check_audio(B, L, training, 96, dtype)


@pytest.mark.parametrize("embed,training,dtype", [(32, True, torch.float32), (160, False, torch.bfloat16)], ids=["NJ1", "NJ3-lanes-past-C"])
def test_audio_gradients_other_widths(embed, training, dtype):
    """embed 32: one channel per lane and half the lanes past C; embed 160: three channels per lane, lanes 32 .. 63 past C in the third"""
    _check_audio(3, 5000, training, embed, dtype)


def test_carried_accumulators():
    """More four-token groups than the launch has waves: B = 8 clips are 8 x 4096 = 32768 tokens = 8192 groups.  The launcher asks for one
    workgroup (4 waves) per 4 groups, 2048, and takes min(2048, resident capacity, 1024 workspace rows).  `patch_embed_bwd_k<1, audio, 2>`
    holds 157 VGPRs = 3 workgroups per CU, so the capacity of 256 CUs is 768 workgroups = 3072 waves: 2 or 3 groups per wave.  Whatever
    the capacity, the 1024 workspace rows cap the grid at 4096 waves, so every wave runs its loop at least twice (8192 / 4096), carrying
    its register accumulators and its LDS bins from one group to the next."""
    lib = dgsct_amd.default_lib()
    rows = lib.patch_embed_params_ws_floats(ops._lib.PATCH_AUDIO, 8, 1, 256, 256, 96) // (19 * 96 + 128)
    assert rows == 1024 and 8 * 4096 // 4 >= 2 * 4 * rows
    _check_audio(8, 3200, True, 96, torch.float32)


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,C", [((2, 3, 32, 32), 128), ((1, 1, 4, 12), 96), ((3, 1, 20, 12), 192)], ids=["rgb", "3-tokens", "mono192"])
def test_image_gradients(shape, C, in_dtype):
    img = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(in_dtype)
    m = R.randomise(PatchEmbed(shape[2:], in_chans=shape[1], embed_dim=C, out_dtype=torch.float32, trainable=True, fused=True), 8)
    n = shape[2] * shape[3] // 16
    cot = cotangent((shape[0], n, C))
    ref, tok64 = image_grads64(img, m.state_dict(), cot)
    m = m.to(DEV)
    tok = m(img.to(DEV))
    assert fp32_err(tok, tok64) < 1e-3
    tok.backward(cot.to(DEV))
    for k in FOUR:
        err = fp32_err(dict(m.named_parameters())[k].grad, ref[k])
        print(f"image {shape} C={C} {in_dtype} {k}: {err:.3e}")
        assert err < 1e-3, k


def _raw_backward(lib, mode, x, T, C, in_chans, H, W, bn, params, dout, fill):
    """one dgsct_patch_embed_backward_params call on outputs and a workspace pre-filled with `fill`"""
    f32 = dict(dtype=torch.float32, device=DEV)
    B = x.shape[0]
    out = [torch.full((C, in_chans, 4, 4), fill, **f32)] + [torch.full((C,), fill, **f32) for _ in range(3)]
    dbn = torch.full((2, 64), fill, **f32) if bn is not None else None
    ws = torch.full((lib.patch_embed_params_ws_floats(mode, B, in_chans, H, W, C),), fill, **f32)
    code = lambda t: ops._lib.F32 if t.dtype == torch.float32 else ops._lib.BF16
    ptr = lambda t: t.data_ptr() if t is not None else None
    scale, shift, pivot = bn if bn is not None else (None, None, None)
    lib.patch_embed_backward_params(mode, code(x), code(dout), B, in_chans, H, W, T, C, x.data_ptr(), ptr(scale), ptr(shift), ptr(pivot),
                                    *(t.data_ptr() for t in params), 1e-5, dout.data_ptr(), *(t.data_ptr() for t in out), ptr(dbn), ws.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out + ([dbn] if dbn is not None else []), ws


def test_raw_call_overwrites_everything_and_repeats_bit_for_bit():
    lib = dgsct_amd.default_lib()
    g = torch.Generator().manual_seed(3)
    nan = float("nan")
    # audio: B = 3, T = 16
    m = _module().to(DEV)
    lm = ops.logmel(_wave(3, 5000)[0].to(DEV), m.logmel_extractor.melW)
    scale, shift = m._bn_affine(None, None, 3 * 16)
    bn = (scale, shift, m.bn0.running_mean.clone())
    pe = m.patch_embed
    params = [t.detach().contiguous() for t in (pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias)]
    dout = torch.randn(3, 4096, 96, generator=g).to(DEV, torch.bfloat16)
    a, ws = _raw_backward(lib, ops._lib.PATCH_AUDIO, lm, 16, 96, 1, 256, 256, bn, params, dout, nan)
    b, _ = _raw_backward(lib, ops._lib.PATCH_AUDIO, lm, 16, 96, 1, 256, 256, bn, params, dout, 7.0)
    assert len(a) == 5 and torch.isfinite(ws).all()
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    # image: 3 tokens, dbn NULL
    p = R.randomise(PatchEmbed((4, 12), in_chans=1, embed_dim=96), 8).to(DEV)
    params = [t.detach().contiguous() for t in (p.proj.weight, p.proj.bias, p.norm.weight, p.norm.bias)]
    img = torch.randn(1, 1, 4, 12, generator=g).to(DEV)
    dout = torch.randn(1, 3, 96, generator=g).to(DEV)
    a, ws = _raw_backward(lib, ops._lib.PATCH_IMAGE, img, 0, 96, 1, 4, 12, None, params, dout, nan)
    b, _ = _raw_backward(lib, ops._lib.PATCH_IMAGE, img, 0, 96, 1, 4, 12, None, params, dout, -3.0)
    assert len(a) == 4 and torch.isfinite(ws).all()
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    with pytest.raises(RuntimeError, match="bn_pivot"):
        _raw_backward(lib, ops._lib.PATCH_AUDIO, lm, 16, 96, 1, 256, 256, (scale, shift, None), params, dout, 0.0)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_fused_against_aten(training):
    x = _wave(3, 5000)[0].to(DEV)
    cot = cotangent((3, 4096, 96)).to(DEV)
    fused = _module(trainable=True, fused=True).to(DEV).train(training)
    aten = _module(trainable=True, fused=False).to(DEV).train(training)
    a, b = fused(x), aten(x)
    assert fp32_err(a, b) < 1e-3 and "PatchEmbedTrain" not in type(b.grad_fn).__name__
    a.backward(cot); b.backward(cot)
    ga, gb = module_grads(fused), module_grads(aten)
    for k in SIX:
        assert fp32_err(ga[k], gb[k]) < 1e-3, k


def test_dispatch_and_errors(monkeypatch):
    lib = dgsct_amd.default_lib()
    calls = []
    real = lib.patch_embed_backward_params
    monkeypatch.setattr(lib, "patch_embed_backward_params", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = _wave(2, 3200)[0].to(DEV)
    m = _module(trainable=True, fused=True).to(DEV).train()
    m(x).sum().backward()
    assert len(calls) == 1                                                   # exactly one call per backward
    p = PatchEmbed(32, in_chans=3, embed_dim=96, trainable=True, fused=True).to(DEV)
    p(torch.zeros(1, 3, 32, 32, device=DEV)).sum().backward()
    assert len(calls) == 2
    # the frozen module, a trainable one without a graph, and a trainable one frozen again never call it
    _module().to(DEV).train()(x)
    with torch.no_grad():
        assert not m(x).requires_grad
    m.requires_grad_(False)
    assert not m(x).requires_grad
    m.requires_grad_(True)
    m.logmel_extractor.melW.requires_grad_(False)
    assert len(calls) == 2
    # fused=None follows the measured policy; fused=False is ATen
    m.fused = m.patch_embed.fused = None
    assert ("PatchEmbedTrain" in type(m(x).grad_fn).__name__) == ("audio" in frontend._KERNELS_FASTER_TRAIN)
    p.fused = None
    assert ("PatchEmbedTrain" in type(p(torch.zeros(1, 3, 32, 32, device=DEV)).grad_fn).__name__) == ("image" in frontend._KERNELS_FASTER_TRAIN)
    m.fused = m.patch_embed.fused = False
    assert "PatchEmbedTrain" not in type(m(x).grad_fn).__name__

    class NoExport:                                                          # a library without the parameter-gradient export
        path = "libstub.so"

        def has_patch_embed_params(self):
            return False

    for mod, inp in ((HTSATFrontEnd(trainable=True, fused=True, lib=NoExport()).to(DEV), x),
                     (PatchEmbed(32, trainable=True, fused=True, lib=NoExport()).to(DEV), torch.zeros(1, 3, 32, 32, device=DEV))):
        with pytest.raises(RuntimeError, match="dgsct_patch_embed_backward_params"):
            mod(inp)
    with pytest.raises(RuntimeError, match="requires grad"):
        _module(trainable=True, fused=True).to(DEV)(x.clone().requires_grad_(True))
    pe = m.patch_embed
    with pytest.raises(RuntimeError, match="may not require grad"):
        ops.patch_embed_train(torch.zeros(1, 3, 32, 32, device=DEV, requires_grad=True), p.proj.weight, p.proj.bias, p.norm.weight, p.norm.bias)
    with pytest.raises(RuntimeError, match="forward-only"):                  # the frozen op keeps refusing parameters that require grad
        ops.patch_embed(torch.zeros(1, 3, 32, 32, device=DEV), p.proj.weight, p.proj.bias, p.norm.weight, p.norm.bias)
    assert pe.proj.weight.requires_grad
